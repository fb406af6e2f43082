// Stateful decoding on the pod server (nos_amd/podserver/program/, ops
// kv_write / rotary_at / sdpa_cache / pos_add / pos_set / argmax) and the
// skinny GEMMs a decode step is made of.  A tenant's K / V cache and its
// position counter live in device memory across requests; every kernel here
// reads the positions ON THE DEVICE, so one captured HIP graph serves every
// step of a generation, and every index a position produces is bounds-checked
// against the buffers (a replay never faults on a bad counter: rows past the
// cache are dropped, table rows clamp).
//
//  * nos_kv_write -- cache[b, pos[b] + s] = x[b, s] (optionally rotated at
//    that position first: the K projection's rotary fused into the write);
//  * nos_rotary_pos -- rotate_half rotary at positions pos[b] + s;
//  * nos_attn_decode -- flash-decoding: query rows at positions pos[b] + i
//    attend the cached keys 0 .. pos[b] + i.  The cache is HBM-bound (per key
//    2 x D loads for G x Sq x 2 D FLOPs, ~2 FLOP/B at Sq = 1): the kernel runs
//    at the cache's own precision with fp32 FMAs on the VALU -- exact for an
//    fp32 cache, more precise than the h3 pipes -- and spends its effort on
//    bandwidth: one workgroup per (sequence, K/V head, 128-key split), every
//    query head of the group (grouped-query) served from one read of the
//    split's keys and values, staged through LDS with 16-byte loads;
//    nos_attn_decode_combine merges the splits (log-sum-exp);
//  * nos_kv_write_q8 / nos_attn_decode_q8 -- the two over int8 caches (D int8 values
//    and one fp32 scale per row): the write quantizes the rows, the attention
//    dequantizes them as it stages a split and is the fp32 cache's code after that;
//  * nos_kv_write_ring(_q8) / nos_attn_decode_ring(_q8) -- the same over ring caches of C slots for a
//    sliding window W (kv_ring.h): position p in slot p % C, query p attends max(0, p - W + 1) .. p;
//  * nos_pos_update -- pos += n / pos = n;
//  * nos_argmax -- greedy next tokens, one wave per row;
//  * nos_sample -- sampled next tokens (temperature, top-k, top-p, seed read
//    from device memory; Gumbel-max over Philox keyed on the position);
//  * nos_seen_mark / nos_penalize / nos_stop_step -- stop ids and the repetition penalty of a
//    stopping tenant: the bitmap of a row's tokens, the penalised logits, and the closing step
//    (pad finished rows, hold their counters, mark rows that drew a stop id);
//  * nos_hist_write / nos_spec_step -- speculative decoding: the token history of each row and a
//    verify step's close (accept the drafts the model confirmed, advance the counter by that
//    many, look the next drafts up in the row's own history);
//  * nos_gemv -- y = act(r x W^T + b) + R for M <= 8 rows (a decode step's
//    every GEMM): weight-streaming, each wave two output columns, lanes over
//    K with 16-byte weight loads, x rows in LDS (optionally RMS-normalised in
//    the prologue: RMSNorm folded into the GEMM, gamma in W), exact fp32 math;
//  * nos_gemv_q8 / nos_gemv_mx4 -- the same over int8 rows with a scale per row and over
//    MXFP4 blocks (4-bit E2M1 codes, an E8M0 scale byte per 32 k): weight-only storage
//    formats, fp32 math on the dequantized values.
#include <float.h>
#include <math.h>

#include "common.h"
#include "epilogue.h"
#include "kv_ring.h"

namespace {

// EPI_GLU (epilogue.h): SwiGLU in the merged gate-up GEMV's epilogue, each wave's two columns being n and n + Nh

__device__ __forceinline__ float ldf(const void* p, long long i, int bf) {
  return bf ? nos::bf16_to_f32(static_cast<const unsigned short*>(p)[i]) : static_cast<const float*>(p)[i];
}

__device__ __forceinline__ void stf(void* p, long long i, float v, int bf) {
  if (bf)
    static_cast<unsigned short*>(p)[i] = nos::f32_to_bf16(v);
  else
    static_cast<float*>(p)[i] = v;
}

// 4 consecutive elements (16-byte fp32 or 8-byte bf16 load) as floats
__device__ __forceinline__ float4 ld4(const void* p, long long i, int bf) {
  if (bf) {
    const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(p) + i);
    return float4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                  __uint_as_float(u.y & 0xffff0000u)};
  }
  return *reinterpret_cast<const float4*>(static_cast<const float*>(p) + i);
}

// the same 4 elements split into the load and the conversion: a batch of loads stays in
// flight whatever the dtype (ld4's bf16 path converts inside its branch, so each of its
// loads waited for its data before the next one issued)
__device__ __forceinline__ uint4 ld4raw(const void* p, long long i, int bf) {
  if (bf) {
    const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(p) + i);
    return uint4{u.x, u.y, 0u, 0u};
  }
  return *reinterpret_cast<const uint4*>(static_cast<const float*>(p) + i);
}

__device__ __forceinline__ float4 cvt4(uint4 r, int bf) {
  if (bf)
    return float4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                  __uint_as_float(r.y & 0xffff0000u)};
  return float4{__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
}

// ------------------------------------------------------------------ int8 K / V cache rows
// A cache row (one (sequence, position, K/V head) vector of D values) of an int8 cache is D int8
// values and one fp32 scale, the int8 weights' rule on the row in fp32: scale = max|row| / 127 (1 for
// an all-zero row), q = clip(rint(row / scale), -127, 127); the value the cache holds is (float)q x
// scale, one rounding.  A wave quantizes a row: lane d < D / 2 holds the rotate_half pair (d, d + D/2).
__device__ __forceinline__ float4 q8_cvt4(unsigned v) {
  return float4{(float)(int)(signed char)(v & 255u), (float)(int)(signed char)((v >> 8) & 255u),
                (float)(int)(signed char)((v >> 16) & 255u), (float)(int)(signed char)(v >> 24)};
}

// the wave's row (x0, x1 per lane; 0 in the lanes past D / 2) -> its scale and this lane's two values
__device__ __forceinline__ float q8_row(float x0, float x1, int& q0, int& q1) {
  const float amax = nos::wave_max(fmaxf(fabsf(x0), fabsf(x1)));
  const float s = amax > 0.f ? amax / 127.f : 1.f;
  q0 = (int)fminf(fmaxf(rintf(x0 / s), -127.f), 127.f);
  q1 = (int)fminf(fmaxf(rintf(x1 / s), -127.f), 127.f);
  return s;
}

// the row's D bytes leave the wave as D / 4 dword stores: lane l < D / 4 gathers elements 4 l .. 4 l + 3
// (element e sits in lane e % (D / 2), half e / (D / 2)) from the lanes' packed pairs; lane 0 the scale
template <int D>
__device__ __forceinline__ void q8_row_store(signed char* __restrict__ row, float* __restrict__ scale, float s, int q0,
                                             int q1, int lane) {
  const int pk = (q0 & 255) | ((q1 & 255) << 8);
  unsigned w = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (4 * lane + i) % D;
    const int t = __shfl(pk, e % (D / 2), 64);
    w |= (unsigned)((e >= D / 2 ? t >> 8 : t) & 255) << (8 * i);
  }
  if (lane < D / 4) reinterpret_cast<unsigned*>(row)[lane] = w;
  if (lane == 0) *scale = s;
}

// ------------------------------------------------------------------ kv_write / rotary at device positions
// one thread per (b, s, h, d < D/2) pair (d, d + D/2): the rotate_half pair
// a fused rotary needs; without tables it just copies both elements
// one K / V pair per launch: blockIdx.y 0 = (x, cache) with the rotary tables
// (K), 1 = (x2, cache2) plain (V; x2 == nullptr: a single write)
struct KvPair {
  const void* x2;
  int ldx2;
  long long bsx2;
  void* cache2;
};

// RING: the cache is a ring of L slots (kv_ring.h): position p goes to slot p % L, positions outside
// [0, limit) are dropped; the rotary tables are read at the position, not the slot
template <bool RING>
__device__ __forceinline__ void kv_write_rows(const void* __restrict__ x, int xbf, int ldx, long long bsx,
                                              void* __restrict__ cache, int cbf, const int* __restrict__ pos,
                                              const float* __restrict__ cs, const float* __restrict__ sn, int R,
                                              int B, int S, int H, int D, int L, KvPair v2, int limit) {
  if (blockIdx.y == 1) {  // the V half: its own rows, no rotation
    x = v2.x2;
    ldx = v2.ldx2;
    bsx = v2.bsx2;
    cache = v2.cache2;
    cs = sn = nullptr;
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int hd = D / 2;
  if (i >= (long long)B * S * H * hd) return;
  const int d = (int)(i % hd);
  long long r = i / hd;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % S), b = (int)(r / S);
  const int p = pos[b] + s;
  int row = p;  // the cache row of position p
  if constexpr (RING) {
    row = nos::ring_slot(p, L, limit);
    if (row < 0) return;  // outside [0, limit): dropped before any address is formed from it
  } else {
    if (p < 0 || p >= L) return;  // past the cache: dropped (the server reports the overflow)
  }
  const long long xo = b * bsx + (long long)s * ldx + (long long)h * D;
  float x0 = ldf(x, xo + d, xbf), x1 = ldf(x, xo + d + hd, xbf);
  if (cs != nullptr) {
    const long long t = (long long)min(p, R - 1) * D;
    const float y0 = fmaf(x0, cs[t + d], -x1 * sn[t + d]);
    const float y1 = fmaf(x1, cs[t + d + hd], x0 * sn[t + d + hd]);
    x0 = y0;
    x1 = y1;
  }
  const long long co = (((long long)b * L + row) * H + h) * D;
  stf(cache, co + d, x0, cbf);
  stf(cache, co + d + hd, x1, cbf);
}

__global__ __launch_bounds__(256) void kv_write_kernel(const void* __restrict__ x, int xbf, int ldx, long long bsx,
                                                       void* __restrict__ cache, int cbf, const int* __restrict__ pos,
                                                       const float* __restrict__ cs, const float* __restrict__ sn,
                                                       int R, int B, int S, int H, int D, int L, KvPair v2) {
  kv_write_rows<false>(x, xbf, ldx, bsx, cache, cbf, pos, cs, sn, R, B, S, H, D, L, v2, 0);
}

__global__ __launch_bounds__(256) void kv_write_ring_kernel(const void* __restrict__ x, int xbf, int ldx,
                                                            long long bsx, void* __restrict__ cache, int cbf,
                                                            const int* __restrict__ pos, const float* __restrict__ cs,
                                                            const float* __restrict__ sn, int R, int B, int S, int H,
                                                            int D, int C, KvPair v2, int limit) {
  kv_write_rows<true>(x, xbf, ldx, bsx, cache, cbf, pos, cs, sn, R, B, S, H, D, C, v2, limit);
}

// kv_write into an int8 cache: one wave per (b, s, h) row -- rotate (K), the row's scale across the
// lanes, quantize, D / 4 dword stores and the scale (q8_row_store); deq (optional, [B, S, H, D] fp32):
// the row as the cache now holds it, for a prefill that attends these rows with the flash kernel
struct KvPairQ8 {
  const float* x2;
  int ldx2;
  long long bsx2;
  signed char* cache2;
  float* scales2;
  float* deq2;
};

template <int D, bool RING>
__device__ __forceinline__ void kv_write_q8_rows(const float* __restrict__ x, int ldx, long long bsx,
                                                 signed char* __restrict__ cache, float* __restrict__ scales,
                                                 float* __restrict__ deq, const int* __restrict__ pos,
                                                 const float* __restrict__ cs, const float* __restrict__ sn, int R,
                                                 int B, int S, int H, int L, KvPairQ8 v2, int limit) {
  if (blockIdx.y == 1) {  // the V half: its own rows, no rotation
    x = v2.x2;
    ldx = v2.ldx2;
    bsx = v2.bsx2;
    cache = v2.cache2;
    scales = v2.scales2;
    deq = v2.deq2;
    cs = sn = nullptr;
  }
  constexpr int hd = D / 2;
  const int lane = threadIdx.x & 63;
  long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // the wave's row
  if (r >= (long long)B * S * H) return;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % S), b = (int)(r / S);
  const int p = pos[b] + s;
  int crow = p;  // the cache row of position p
  if constexpr (RING) {
    crow = nos::ring_slot(p, L, limit);
    if (crow < 0) return;  // outside [0, limit): dropped (the whole wave)
  } else {
    if (p < 0 || p >= L) return;  // past the cache: dropped (the whole wave)
  }
  float x0 = 0.f, x1 = 0.f;
  if (lane < hd) {
    const long long xo = b * bsx + (long long)s * ldx + (long long)h * D;
    x0 = x[xo + lane];
    x1 = x[xo + lane + hd];
    if (cs != nullptr) {
      const long long t = (long long)min(p, R - 1) * D;
      const float y0 = fmaf(x0, cs[t + lane], -x1 * sn[t + lane]);
      const float y1 = fmaf(x1, cs[t + lane + hd], x0 * sn[t + lane + hd]);
      x0 = y0;
      x1 = y1;
    }
  }
  int q0, q1;
  const float sc = q8_row(x0, x1, q0, q1);
  const long long row = ((long long)b * L + crow) * H + h;
  q8_row_store<D>(cache + row * D, scales + row, sc, q0, q1, lane);
  if (deq != nullptr && lane < hd) {
    const long long yo = (((long long)b * S + s) * H + h) * D;
    deq[yo + lane] = (float)q0 * sc;
    deq[yo + lane + hd] = (float)q1 * sc;
  }
}

template <int D>
__global__ __launch_bounds__(256) void kv_write_q8_kernel(const float* __restrict__ x, int ldx, long long bsx,
                                                          signed char* __restrict__ cache, float* __restrict__ scales,
                                                          float* __restrict__ deq, const int* __restrict__ pos,
                                                          const float* __restrict__ cs, const float* __restrict__ sn,
                                                          int R, int B, int S, int H, int L, KvPairQ8 v2) {
  kv_write_q8_rows<D, false>(x, ldx, bsx, cache, scales, deq, pos, cs, sn, R, B, S, H, L, v2, 0);
}

template <int D>
__global__ __launch_bounds__(256) void kv_write_q8_ring_kernel(
    const float* __restrict__ x, int ldx, long long bsx, signed char* __restrict__ cache, float* __restrict__ scales,
    float* __restrict__ deq, const int* __restrict__ pos, const float* __restrict__ cs, const float* __restrict__ sn,
    int R, int B, int S, int H, int C, KvPairQ8 v2, int limit) {
  kv_write_q8_rows<D, true>(x, ldx, bsx, cache, scales, deq, pos, cs, sn, R, B, S, H, C, v2, limit);
}

__global__ __launch_bounds__(256) void rotary_pos_kernel(const void* __restrict__ x, int ldx, long long bsx,
                                                         void* __restrict__ y, const int* __restrict__ pos,
                                                         const float* __restrict__ cs, const float* __restrict__ sn,
                                                         int R, int B, int S, int H, int D, int bf) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int hd = D / 2;
  if (i >= (long long)B * S * H * hd) return;
  const int d = (int)(i % hd);
  long long r = i / hd;
  const int h = (int)(r % H);
  r /= H;
  const int s = (int)(r % S), b = (int)(r / S);
  const int p = min(max(pos[b] + s, 0), R - 1);
  const long long xo = b * bsx + (long long)s * ldx + (long long)h * D;
  const float x0 = ldf(x, xo + d, bf), x1 = ldf(x, xo + d + hd, bf);
  const long long t = (long long)p * D;
  const long long yo = (((long long)b * S + s) * H + h) * D;
  stf(y, yo + d, fmaf(x0, cs[t + d], -x1 * sn[t + d]), bf);
  stf(y, yo + d + hd, fmaf(x1, cs[t + d + hd], x0 * sn[t + d + hd]), bf);
}

// ------------------------------------------------------------------ decode attention
constexpr int KC = 128;      // keys per split (one workgroup)
constexpr int MAXR = 32;     // query rows (G x Sq) per launch

// workgroup (b, kvh, split): rows r = qi * G + g (query token qi of Sq, query
// head kvh * G + g); q rows scaled (and rotated) into LDS, the split's keys
// into LDS, scores -> per-row max / sum -> probabilities in LDS, the split's
// values into LDS, P V; the partial (acc[D], m, l) of every row to ws
// the step's own K / V rows (written into the caches by this kernel instead of a
// kv_write launch): token t of batch b at k + b * bsk + t * ldk + h * D (V alike),
// cache row pos[b] + t; n = 0: none (the caches already hold them)
struct Fresh {
  const void* k = nullptr;
  const void* v = nullptr;
  void* kc = nullptr;
  void* vc = nullptr;
  long long bsk = 0, bsv = 0;
  int ldk = 0, ldv = 0, bf = 0, n = 0;
};

// row r of group bk = (b, kvh): out[b, q0 + qi, h, d] = sum_s e^(m_s - M) acc_s / sum_s
// e^(m_s - M) l_s over the NS splits' partials (splits with l = 0 skipped)
template <int D>
__device__ __forceinline__ void decode_combine_row(const float* __restrict__ ws, void* __restrict__ o, int obf,
                                                   int bk, int r, int d, int NS, int G, int R, int H, int Hkv,
                                                   int Sq_total, int q0) {
  const int kvh = bk % Hkv, b = bk / Hkv;
  const int qi = r / G, h = kvh * G + r % G;
  float M = -INFINITY;
  for (int s = 0; s < NS; ++s) {
    const float* p = ws + ((long long)(bk * NS + s) * R + r) * (D + 2);
    if (p[D + 1] > 0.f) M = fmaxf(M, p[D]);
  }
  float num = 0.f, den = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float* p = ws + ((long long)(bk * NS + s) * R + r) * (D + 2);
    if (p[D + 1] > 0.f) {
      const float w = __expf(p[D] - M);
      num = fmaf(w, p[d], num);
      den = fmaf(w, p[D + 1], den);
    }
  }
  const long long oo = (((long long)b * Sq_total + q0 + qi) * H + h) * D + d;
  stf(o, oo, den > 0.f ? num / den : 0.f, obf);
}

// the combine launch folded into the decode launch (sync != null): each workgroup
// publishes its partial (device-scope fence: the splits run on different XCDs, each
// with its own L2), counts itself in on its group's counter, and the group's last
// workgroup combines the NS partials and zeroes the counter for the next launch.
// No workgroup waits on another, so the grid drains whatever the order.
template <int D>
__device__ __forceinline__ void decode_combine_last(const float* __restrict__ ws, int* __restrict__ sync,
                                                    void* __restrict__ o, int obf, int bk, int NS, int G, int R,
                                                    int H, int Hkv, int Sq_total, int q0, int tid) {
  if (sync == nullptr) return;
  __shared__ int last;
  __threadfence();
  __syncthreads();
  if (tid == 0) last = atomicAdd(&sync[bk], 1) == NS - 1;
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (int e = tid; e < R * D; e += 256) decode_combine_row<D>(ws, o, obf, bk, e / D, e % D, NS, G, R, H, Hkv, Sq_total, q0);
  if (tid == 0) atomicExch(&sync[bk], 0);
}

// the row scales [B, L, Hkv] of int8 caches (CBF == 2): a kernel argument only of that instantiation
template <int CBF>
struct CacheScales {};
template <>
struct CacheScales<2> {
  float* k;
  float* v;
};

// a sliding window over ring caches (RING): a kernel argument only of those instantiations
template <bool RING>
struct RingArgs {};
template <>
struct RingArgs<true> {
  int W;      // the window: the query at p attends the positions max(0, p - W + 1) .. p
  int limit;  // positions >= limit are not stored (the rows of the rotary tables)
};

// CBF: the cache kind -- 0 fp32, 1 bf16, 2 int8 rows with a scale each (dequantized as they are staged
// into the fp32 LDS tile: a quarter of the fp32 cache's bytes from HBM, the same arithmetic after it)
// RING: the caches are rings of L = C slots (kv_ring.h) and the queries attend a window.  A split is a
// range of slots; the position a slot holds follows from the step's last position pmax = pos[b] +
// Sq_total - 1, the same in every launch of the step.  nk counts the split's slots up to the last one
// some row of the launch sees; the slots below it that no row sees are staged as zeros without a load
// (stale or never written: they must not reach P V as 0 x garbage).  With nothing hidden and nothing
// wrapped the split's arithmetic is the plain kernel's, in its order.
template <int D, int CBF, bool RING = false>
__global__ __launch_bounds__(256) void attn_decode_kernel(
    const void* __restrict__ q, int qbf, int ldq, long long bsq, const void* __restrict__ kc,
    const void* __restrict__ vc, int /*cbf = CBF*/, const int* __restrict__ pos, const float* __restrict__ cs,
    const float* __restrict__ sn, int Rtab, float* __restrict__ ws, int B, int H, int Hkv, int Sq, int q0, int L,
    int NS, float scale, Fresh fr, int* __restrict__ sync, void* __restrict__ o, int obf, int Sq_total,
    CacheScales<CBF> csc, RingArgs<RING> rg) {
  constexpr int cbf = CBF;   // the cache dtype fixed at compile time: no per-load dtype branch
  constexpr int DP = D + 4;  // padded LDS row (16-byte reads of consecutive rows hit distinct banks)
  __shared__ __attribute__((aligned(16))) float qs[MAXR * D];
  __shared__ __attribute__((aligned(16))) float kv[KC * DP];
  __shared__ float sc[MAXR * KC];
  __shared__ float mrow[MAXR], lrow[MAXR];
  float* rsc = nullptr;  // int8 caches: the split's K row scales, then its V row scales
  if constexpr (CBF == 2) {
    __shared__ float rsc_[2 * KC];
    rsc = rsc_;
  }
  const int G = H / Hkv, R = G * Sq;
  const int split = blockIdx.x % NS, bk = blockIdx.x / NS;
  const int kvh = bk % Hkv, b = bk / Hkv;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int p0 = pos[b] + q0;                              // position of query row qi = 0 of this launch
  const int k0 = split * KC;
  // RING: a counter outside [0, limit) is bad (nothing written, every split dead); the positions the
  // rows of this launch see are vlo .. vhi, and slot s holds one of them iff seen(s)
  bool good = true;
  int pmax = 0, vlo = 0, vhi = -1, nk;
  if constexpr (RING) {
    good = pos[b] >= 0 && pos[b] < rg.limit;
    pmax = pos[b] + Sq_total - 1;
    vhi = p0 + Sq - 1;
    vlo = nos::ring_oldest(p0, pmax, L, rg.W);
    nk = good ? nos::ring_split_rows(k0, min(KC, L - k0), vlo, vhi, L) : 0;
  } else {
    const int kend = min(p0 + Sq, L);                      // keys 0 .. kend - 1 are visible to some row
    nk = min(KC, kend - k0);
  }
  auto seen = [&](int s) {
    const int a = nos::ring_position(s, pmax, L);
    return a >= vlo && a <= vhi;
  };
  // row j of the split is loaded (else staged as zeros)
  auto has = [&](int j) {
    if constexpr (RING)
      return j < nk && seen(k0 + j);
    else
      return j < nk;
  };
  // the cache row of the step's fresh row t (RING: -1 for a dropped row; else the caller drops rows >= L)
  auto fresh_slot = [&](int t) {
    if constexpr (RING)
      return nos::ring_slot(pos[b] + t, L, rg.limit);
    else
      return pos[b] + t;
  };
  float* const out = ws + (long long)blockIdx.x * R * (D + 2);
  const long long cstride = (long long)Hkv * D;  // cache row (token) stride
  // the first launch of a step writes the step's fresh K (rotated) / V rows that fall in
  // this split's key range into the caches -- every split, empty or not, so a later
  // launch (query rows q0 > 0) and the next step read them from the cache
  const bool fresh = fr.n > 0 && q0 == 0 && pos[b] >= 0 && good;
  auto fresh_row = [&](int t, int d, bool isk, float& x0, float& x1) {
    const void* src = isk ? fr.k : fr.v;
    const long long o = (long long)b * (isk ? fr.bsk : fr.bsv) + (long long)t * (isk ? fr.ldk : fr.ldv) +
                        (long long)kvh * D;
    x0 = ldf(src, o + d, fr.bf);
    x1 = ldf(src, o + d + D / 2, fr.bf);
    if (isk && cs != nullptr) {
      const long long tt = (long long)min(pos[b] + t, Rtab - 1) * D;
      const float y0 = fmaf(x0, cs[tt + d], -x1 * sn[tt + d]);
      const float y1 = fmaf(x1, cs[tt + d + D / 2], x0 * sn[tt + d + D / 2]);
      x0 = y0;
      x1 = y1;
    }
    if (CBF == 1) {  // a bf16 cache holds the row rounded: the step attends what every later read of the cache sees
      x0 = nos::bf16_to_f32(nos::f32_to_bf16(x0));
      x1 = nos::bf16_to_f32(nos::f32_to_bf16(x1));
    }
  };
  // an int8 cache holds the row quantized, which takes the row's maximum: one wave per fresh row,
  // lane d < D / 2 its pair; every lane gets the scale
  auto fresh_row_q8 = [&](int t, bool isk, int& q0_, int& q1_) {
    float x0 = 0.f, x1 = 0.f;
    if (lane < D / 2) fresh_row(t, lane, isk, x0, x1);
    return q8_row(x0, x1, q0_, q1_);
  };
  // the split's K and V rows are loaded into registers first, every load of both in flight
  // at once; the fresh-row stores, the q staging and the scores overlap their latency (a
  // fresh row's stale cache value is replaced by the overlay below)
  const long long cbase = ((long long)b * L + k0) * cstride + (long long)kvh * D;
  // a thread's piece: 4 elements (16 bytes of fp32, 8 of bf16), or 16 bytes = 16 values of an int8 row
  constexpr int EPP = CBF == 2 ? 16 : 4;
  constexpr int PER = KC * (D / EPP) / 256;
  static_assert(PER * 256 == KC * (D / EPP), "whole pieces per thread");
  uint4 kr[PER], vr[PER];
  float rs = 0.f;  // int8: thread j < KC the scale of K row j, thread KC + j of V row j
  const bool live = nk > 0 && p0 >= 0;
  if (live) {
    if constexpr (CBF == 2) {
      const int j = tid & (KC - 1);
      if (has(j)) rs = (tid < KC ? csc.k : csc.v)[((long long)b * L + k0 + j) * Hkv + kvh];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, j = e / (D / EPP), d4 = (e % (D / EPP)) * EPP;
      if constexpr (CBF == 2)
        kr[u] = has(j) ? *reinterpret_cast<const uint4*>(static_cast<const signed char*>(kc) + cbase + j * cstride + d4)
                       : uint4{0u, 0u, 0u, 0u};
      else
        kr[u] = has(j) ? ld4raw(kc, cbase + j * cstride + d4, cbf) : uint4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, j = e / (D / EPP), d4 = (e % (D / EPP)) * EPP;
      if constexpr (CBF == 2)
        vr[u] = has(j) ? *reinterpret_cast<const uint4*>(static_cast<const signed char*>(vc) + cbase + j * cstride + d4)
                       : uint4{0u, 0u, 0u, 0u};
      else
        vr[u] = has(j) ? ld4raw(vc, cbase + j * cstride + d4, cbf) : uint4{0u, 0u, 0u, 0u};
    }
  }
  if constexpr (CBF == 2) {
    if (fresh) {
      for (int r = wid; r < 2 * fr.n; r += 4) {  // wave-uniform: the whole wave takes or skips a row
        const int isv = r >= fr.n, t = isv ? r - fr.n : r, jabs = fresh_slot(t);
        if (jabs < k0 || jabs >= k0 + KC || jabs >= L) continue;
        int q0_, q1_;
        const float s = fresh_row_q8(t, !isv, q0_, q1_);
        const long long row = ((long long)b * L + jabs) * Hkv + kvh;
        q8_row_store<D>(static_cast<signed char*>(isv ? fr.vc : fr.kc) + row * D, (isv ? csc.v : csc.k) + row, s, q0_,
                        q1_, lane);
      }
    }
  } else if (fresh) {
    for (int e = tid; e < 2 * fr.n * (D / 2); e += 256) {
      const int isv = e >= fr.n * (D / 2), ee = isv ? e - fr.n * (D / 2) : e;
      const int t = ee / (D / 2), d = ee % (D / 2), jabs = fresh_slot(t);
      if (jabs < k0 || jabs >= k0 + KC || jabs >= L) continue;
      float x0, x1;
      fresh_row(t, d, !isv, x0, x1);
      void* cache = isv ? fr.vc : fr.kc;
      const long long co = ((long long)b * L + jabs) * cstride + (long long)kvh * D;
      stf(cache, co + d, x0, cbf);
      stf(cache, co + d + D / 2, x1, cbf);
    }
  }
  // the fresh rows this split attends come from the registers' source, not the cache
  // (its stores above may still be in flight): staged over the cache's rows, at the cache's
  // precision (fresh_row)
  // the split row that fresh row t is staged over (outside 0 .. nk - 1: none)
  auto fresh_at = [&](int t) {
    if constexpr (RING) {
      const int s = fresh_slot(t);
      return s < 0 ? -1 : s - k0;
    } else {
      return pos[b] + t - k0;
    }
  };
  auto overlay = [&](bool isk) {
    if (!fresh) return;
    __syncthreads();
    if constexpr (CBF == 2) {  // what the stores above put into the cache, dequantized
      for (int t = wid; t < fr.n; t += 4) {
        const int j = fresh_at(t);
        if (j < 0 || j >= nk) continue;
        int q0_, q1_;
        const float s = fresh_row_q8(t, isk, q0_, q1_);
        if (lane < D / 2) {
          kv[j * (D + 4) + lane] = (float)q0_ * s;
          kv[j * (D + 4) + lane + D / 2] = (float)q1_ * s;
        }
      }
      return;
    }
    for (int e = tid; e < fr.n * (D / 2); e += 256) {
      const int t = e / (D / 2), d = e % (D / 2), j = fresh_at(t);
      if (j < 0 || j >= nk) continue;
      float x0, x1;
      fresh_row(t, d, isk, x0, x1);
      kv[j * (D + 4) + d] = x0;
      kv[j * (D + 4) + d + D / 2] = x1;
    }
  };
  if (!live) {  // an empty split (or a bad counter): l = 0, skipped by the combine
    for (int r = tid; r < R; r += 256) {
      out[r * (D + 2) + D] = -INFINITY;
      out[r * (D + 2) + D + 1] = 0.f;
    }
    decode_combine_last<D>(ws, sync, o, obf, bk, NS, G, R, H, Hkv, Sq_total, q0, tid);
    return;
  }
  // q rows -> LDS, times the softmax scale (rotated at their positions first)
  for (int e = tid; e < R * (D / 2); e += 256) {
    const int r = e / (D / 2), d = e % (D / 2);
    const int qi = r / G, g = r % G, h = kvh * G + g;
    const long long qo = b * bsq + (long long)(q0 + qi) * ldq + (long long)h * D;
    float x0 = ldf(q, qo + d, qbf), x1 = ldf(q, qo + d + D / 2, qbf);
    if (cs != nullptr) {
      const long long t = (long long)min(max(p0 + qi, 0), Rtab - 1) * D;
      const float y0 = fmaf(x0, cs[t + d], -x1 * sn[t + d]);
      const float y1 = fmaf(x1, cs[t + d + D / 2], x0 * sn[t + d + D / 2]);
      x0 = y0;
      x1 = y1;
    }
    qs[r * D + d] = x0 * scale;
    qs[r * D + d + D / 2] = x1 * scale;
  }
  // the split's rows -> LDS from the registers loaded at the start (rows past nk zero)
  // (int8: each value times its row's scale, rsc + sbase; rows past nk have zero bytes and a zero scale)
  auto stage = [&](const uint4 (&v)[PER], int sbase) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + 256 * u, j = e / (D / EPP), d4 = (e % (D / EPP)) * EPP;
      if constexpr (CBF == 2) {
        const float s = rsc[sbase + j];
        const unsigned wd[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 f = q8_cvt4(wd[i]);
          *reinterpret_cast<float4*>(&kv[j * DP + d4 + 4 * i]) = float4{f.x * s, f.y * s, f.z * s, f.w * s};
        }
      } else {
        *reinterpret_cast<float4*>(&kv[j * DP + d4]) = cvt4(v[u], cbf);
      }
    }
  };
  if constexpr (CBF == 2) {
    rsc[tid] = rs;
    __syncthreads();
  }
  stage(kr, 0);
  overlay(true);
  __syncthreads();
  // scores: thread -> key j, rows of one parity
  {
    const int j = tid & (KC - 1), rh = tid >> 7;
    const int jabs = k0 + j;
    // two partial dot products per row (even / odd float4s of d): at decode's few
    // rows (G x 1) one chain of D dependent FMAs per row was latency-bound
    float acc[MAXR / 2], acc2[MAXR / 2];
#pragma unroll
    for (int i = 0; i < MAXR / 2; ++i) acc[i] = acc2[i] = 0.f;
    for (int d4 = 0; d4 < D; d4 += 8) {
      const float4 kk = *reinterpret_cast<const float4*>(&kv[j * DP + d4]);
      const float4 k2 = *reinterpret_cast<const float4*>(&kv[j * DP + d4 + 4]);
#pragma unroll
      for (int i = 0; i < MAXR / 2; ++i) {
        const int r = rh + 2 * i;
        if (r < R) {
          const float4 qq = *reinterpret_cast<const float4*>(&qs[r * D + d4]);
          const float4 q2 = *reinterpret_cast<const float4*>(&qs[r * D + d4 + 4]);
          acc[i] = fmaf(qq.x, kk.x, fmaf(qq.y, kk.y, fmaf(qq.z, kk.z, fmaf(qq.w, kk.w, acc[i]))));
          acc2[i] = fmaf(q2.x, k2.x, fmaf(q2.y, k2.y, fmaf(q2.z, k2.z, fmaf(q2.w, k2.w, acc2[i]))));
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MAXR / 2; ++i) acc[i] += acc2[i];
#pragma unroll
    for (int i = 0; i < MAXR / 2; ++i) {
      const int r = rh + 2 * i;
      if (r < R) {
        const int qpos = p0 + r / G;  // causal: this row sees keys <= its position
        if constexpr (RING)
          sc[r * KC + j] = (j < nk && nos::ring_visible(jabs, qpos, pmax, L, rg.W)) ? acc[i] : -INFINITY;
        else
          sc[r * KC + j] = (j < nk && jabs <= qpos) ? acc[i] : -INFINITY;
      }
    }
  }
  __syncthreads();
  // per-row max / sum over the split; probabilities back into sc
  for (int r = wid; r < R; r += 4) {
    const float s0 = sc[r * KC + lane], s1 = sc[r * KC + lane + 64];
    const float m = nos::wave_max(fmaxf(s0, s1));
    const float e0 = m == -INFINITY ? 0.f : __expf(s0 - m), e1 = m == -INFINITY ? 0.f : __expf(s1 - m);
    sc[r * KC + lane] = e0;
    sc[r * KC + lane + 64] = e1;
    const float l = nos::wave_sum(e0 + e1);
    if (lane == 0) {
      mrow[r] = m;
      lrow[r] = l;
    }
  }
  __syncthreads();  // every wave is done with the keys
  stage(vr, KC);
  overlay(false);
  __syncthreads();
  // P V: thread -> column d, rows of one residue
  {
    constexpr int RS = 256 / D;  // rows in parallel
    const int d = tid % D, r0 = tid / D;
    for (int r = r0; r < R; r += RS) {
      // four partial sums: a chain of nk dependent FMAs (each behind two LDS reads) was
      // latency-bound; keys past nk hold P = 0 and zero V rows, so the unrolled tail adds 0
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      for (int j = 0; j < nk; j += 4) {
        a0 = fmaf(sc[r * KC + j], kv[j * DP + d], a0);
        a1 = fmaf(sc[r * KC + j + 1], kv[(j + 1) * DP + d], a1);
        a2 = fmaf(sc[r * KC + j + 2], kv[(j + 2) * DP + d], a2);
        a3 = fmaf(sc[r * KC + j + 3], kv[(j + 3) * DP + d], a3);
      }
      out[r * (D + 2) + d] = (a0 + a1) + (a2 + a3);
    }
    for (int r = tid; r < R; r += 256) {
      out[r * (D + 2) + D] = mrow[r];
      out[r * (D + 2) + D + 1] = lrow[r];
    }
  }
  decode_combine_last<D>(ws, sync, o, obf, bk, NS, G, R, H, Hkv, Sq_total, q0, tid);
}

// out[b, q0 + qi, h, :] = sum_s e^(m_s - M) acc_s / sum_s e^(m_s - M) l_s over the splits
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(const float* __restrict__ ws, void* __restrict__ o,
                                                                int obf, int B, int H, int Hkv, int Sq, int q0,
                                                                int Sq_total, int NS) {
  const int G = H / Hkv, R = G * Sq;
  const int row = blockIdx.x;  // (b, kvh, r)
  decode_combine_row<D>(ws, o, obf, row / R, row % R, threadIdx.x, NS, G, R, H, Hkv, Sq_total, q0);
}

// ------------------------------------------------------------------ positions, argmax
__global__ void pos_update_kernel(int* __restrict__ pos, int B, int add, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) pos[i] = add ? pos[i] + n : n;
}

// first index of the row maximum (torch.argmax's tie rule); NaN rows give the NaN's index
// (value, index) b better than a: NaN beats numbers (torch.argmax), then the
// larger value, then the smaller index -- the first maximum
__device__ __forceinline__ bool am_better(float bv, int bi, float av, int ai) {
  const bool bn = bv != bv, an = av != av;
  if (bn != an) return bn;
  if (bn) return bi < ai;
  return bv > av || (bv == av && bi < ai);
}

// one workgroup of NT threads per row: 4 independent loads in flight per thread
// per step (a wave per row left a 32000-wide vocabulary row latency-bound at
// ~180 us), wave shuffles, then the waves' winners through LDS
template <int NT>
__global__ __launch_bounds__(NT) void argmax_kernel(const void* __restrict__ x, int bf, int rows, int L, int ldx,
                                                    int* __restrict__ out, int* __restrict__ pos, int pos_n) {
  __shared__ float sv[NT / 64];
  __shared__ int si[NT / 64];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long base = (long long)row * ldx;
  float best = -INFINITY;
  int bi = INT_MAX;
  for (int j0 = tid; j0 < L; j0 += 4 * NT) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * NT;
      v[u] = j < L ? ldf(x, base + j, bf) : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * NT;
      if (j < L && am_better(v[u], j, best, bi)) {
        best = v[u];
        bi = j;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (am_better(ob, oi, best, bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    sv[wid] = best;
    si[wid] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NT / 64; ++w)
      if (am_better(sv[w], si[w], best, bi)) {
        best = sv[w];
        bi = si[w];
      }
    out[row] = bi >= L ? 0 : bi;  // an all -inf row: index 0
    if (pos != nullptr) pos[row] += pos_n;  // the step's position advance folded in (row = sequence)
  }
}

// ------------------------------------------------------------------ stop ids and repetition penalty
// The stopping tenant's control words, read from device memory when a kernel runs (one captured
// graph serves every request): ctl = [penalty fp32 bits, pad_id, n_stop (0..4), stop0 .. stop3, 0].
// All zero: no stop ids, penalty 1.

// seen [B, W] (i32 bitmaps, bit id & 31 of word id >> 5) |= the ids [B, S] of each row; reset: every
// row cleared first.  One workgroup per row, so clear-then-mark is one launch with no ordering
// between workgroups; ids outside [0, vocab) (vocab <= 32 W) are dropped.
__global__ __launch_bounds__(256) void seen_mark_kernel(int* __restrict__ seen, int W, const int* __restrict__ ids,
                                                        int S, long long ld_ids, int vocab, int reset) {
  const int row = blockIdx.x, tid = threadIdx.x;
  int* words = seen + (long long)row * W;
  if (reset) {
    for (int w = tid; w < W; w += 256) words[w] = 0;
    __threadfence();   // the clears reach L2, where the atomics below run, before any of them
    __syncthreads();
  }
  for (int s = tid; s < S; s += 256) {
    const int id = ids[(long long)row * ld_ids + s];
    if (id >= 0 && id < vocab) atomicOr(&words[id >> 5], (int)(1u << (id & 31)));
  }
}

__device__ __forceinline__ float penalized(float x, float p, bool seen) {
  return seen ? (x < 0.f ? x * p : x / p) : x;   // a true division (correctly rounded), as the reference's
}

// out[row, v] = x[row, v] where bit v of the row's bitmap is clear, else x < 0 ? x p : x / p (fp32
// math; bf16 logits rounded once).  x is only read and out is another buffer, so a token seen twice
// is penalised once.  Each thread 4 consecutive logits; a wave covers 256 of them = 8 bitmap words,
// loaded by its lanes 0 .. 7 and handed to the others by a shuffle: one load per 32 logits.
// vec: 16-byte (bf16: 8-byte) loads and stores (the host checked the strides and alignments).
__global__ __launch_bounds__(256) void penalize_kernel(const void* __restrict__ x, int bf, int L, long long ldx,
                                                       void* __restrict__ out, long long ldo,
                                                       const int* __restrict__ seen, int W,
                                                       const int* __restrict__ ctl, int vec) {
  const int row = blockIdx.y, lane = threadIdx.x & 63;
  const long long j = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;   // this thread's first logit
  const long long wbase = (j - 4 * lane) >> 5;                            // the wave's first bitmap word
  unsigned word = 0;
  if (lane < 8 && wbase + lane < W) word = (unsigned)seen[(long long)row * W + wbase + lane];
  word = (unsigned)__shfl((int)word, lane >> 3, 64);
  if (j >= L) return;
  const int cp = ctl[0];
  const float p = cp == 0 ? 1.f : __int_as_float(cp);
  const unsigned bits = p == 1.f ? 0u : (word >> ((lane & 7) * 4)) & 15u;   // penalty 1: an exact copy
  const long long xi = (long long)row * ldx + j, oi = (long long)row * ldo + j;
  if (vec && j + 3 < L) {
    const float4 v = ld4(x, xi, bf);
    const float r0 = penalized(v.x, p, bits & 1u), r1 = penalized(v.y, p, bits & 2u);
    const float r2 = penalized(v.z, p, bits & 4u), r3 = penalized(v.w, p, bits & 8u);
    if (bf) {
      const unsigned lo = (unsigned)nos::f32_to_bf16(r0) | ((unsigned)nos::f32_to_bf16(r1) << 16);
      const unsigned hi = (unsigned)nos::f32_to_bf16(r2) | ((unsigned)nos::f32_to_bf16(r3) << 16);
      *reinterpret_cast<uint2*>(static_cast<unsigned short*>(out) + oi) = uint2{lo, hi};
    } else {
      *reinterpret_cast<float4*>(static_cast<float*>(out) + oi) = float4{r0, r1, r2, r3};
    }
    return;
  }
  for (int u = 0; u < 4 && j + u < L; ++u)
    stf(out, oi + u, penalized(ldf(x, xi + u, bf), p, (bits >> u) & 1u), bf);
}

// A stopping program's closing trio in one launch, one thread per row (mode: which of the three
// run; all = 7).  The row's done flag is read first, then
//  1: ids_out[b] = done ? pad_id : next[b]                      (stop_ids)
//  2: pos[b] += n unless done                                   (pos_add(pos, done))
//  4: done[b] |= id in {stop0 .. stop(n_stop - 1)}              (done_mark; id: what 1 wrote, or next[b])
__global__ void stop_step_kernel(const int* __restrict__ next, int* __restrict__ ids_out, int* __restrict__ pos,
                                 int* __restrict__ done, const int* __restrict__ ctl, int B, int n, int mode) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int d = done[b];
  int id = (mode & 5) ? next[b] : 0;
  if (mode & 1) {
    if (d) id = ctl[1];
    ids_out[b] = id;
  }
  if ((mode & 2) && !d) pos[b] += n;
  if (mode & 4) {
    const int ns = min(max(ctl[2], 0), 4);
    int hit = 0;
    for (int k = 0; k < ns; ++k) hit |= id == ctl[3 + k];
    if (hit) done[b] = d | 1;
  }
}

// ------------------------------------------------------------------ speculative decoding (n-gram drafts)
// hist [B, L]: from base = pos[b] - back on, the first `lead` columns of ids, then the columns of
// tail [B, T] -- with n only its first n[b], and nothing at all for a row whose n[b] <= 0.  One
// workgroup per row; every index is checked against [0, L).
__global__ __launch_bounds__(256) void hist_write_kernel(int* __restrict__ hist, int L, const int* __restrict__ pos,
                                                         int back, const int* __restrict__ ids, int lead,
                                                         long long ld_ids, const int* __restrict__ tail, int T,
                                                         long long ld_tail, const int* __restrict__ n) {
  const int b = blockIdx.x;
  int cnt = T;
  if (n) {
    const int c = n[b];
    if (c <= 0) return;
    cnt = min(c, T);
  }
  const long long base = (long long)pos[b] - back;
  for (int s = threadIdx.x; s < lead + cnt; s += 256) {
    const long long idx = base + s;
    if (idx < 0 || idx >= L) continue;
    hist[(long long)b * L + idx] = s < lead ? ids[b * ld_ids + s] : tail[b * ld_tail + (s - lead)];
  }
}

constexpr int kSpecMaxK = 8;

// A verify step's close, one workgroup per row (mode: which parts run; the whole step = 15).
//  1: m = the step's advance -> n_acc[b].  ids [B, K]: the pending token at p = pos[b] and K - 1
//     drafts; g [B, K]: the model's draw after each.  a = the leading j in 1 .. K - 1 with
//     ids[j] == g[j - 1]; m = min(a + 1, L - 1 - p, end - p if end > 0) floored at 0, end = ctl[0];
//     a p outside [0, L) gives 0.  (Without 1, m is read from n_acc[b].)
//  2: a row with m > 0 writes hist[p] = ids[0], hist[p + 1 .. p + m] = g[0 .. m - 1]
//  4: pos[b] = p + m
//  8: out [B, K] = the next step's input at p' = pos[b] (after 4): the pending token hist[p'],
//     then K - 1 drafts by n-gram lookup -- for n = 3, 2, 1 (each only if p' >= n) the largest
//     t < p' with hist[t - n + 1 .. t] == hist[p' - n + 1 .. p']; the first n with a match wins and
//     draft j is hist[t + j] if t + j <= p', else the pending token (as is every draft without a
//     match).  The threads share the candidates t; each keys its best as (matched length, t) and a
//     block-wide max picks the winner.  A p' outside [0, L): zeros.
// Bounds: m <= L - 1 - p keeps every hist write below L, the lookup reads 0 .. p' < L only, and a
// row with a counter outside [0, L) is left alone (m = 0: no write, the counter unchanged).  The
// words this launch writes are read back from LDS, never from memory.
// The K / V rows p + m .. p + K - 1 the step's body wrote for rejected drafts stay in the caches (int8
// caches: with their scales): attention reads the keys up to its own position only, the next step's
// first query sits at p + m, and each of those rows is rewritten, with its scale, by the step that
// processes its position before any query can reach it.
__global__ __launch_bounds__(256) void spec_step_kernel(int* hist, int L, int* __restrict__ pos,
                                                        const int* __restrict__ ids, const int* __restrict__ g,
                                                        const int* __restrict__ ctl, int* __restrict__ n_acc,
                                                        int* __restrict__ out, int K, int mode) {
  __shared__ int s_new[kSpecMaxK + 1];
  __shared__ int s_at[3];   // p (where s_new starts), the words s_new holds, p'
  __shared__ int s_best[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    const int p = pos[b];
    const bool ok = p >= 0 && p < L;
    int m = 0, wrote = 0;
    if (mode & 1) {
      if (ok) {
        int a = 0;
        while (a + 1 < K && ids[b * K + a + 1] == g[b * K + a]) ++a;
        m = min(a + 1, L - 1 - p);
        const int end = ctl[0];
        if (end > 0) m = min(m, end - p);
        m = max(m, 0);
      }
      n_acc[b] = m;
    } else if (mode & 4) {
      m = n_acc[b];
    }
    if ((mode & 2) && m > 0) {   // mode 2 comes with 1: 0 <= p, p + m <= L - 1, m <= K
      s_new[0] = ids[b * K];
      for (int j = 0; j < m; ++j) s_new[1 + j] = g[b * K + j];
      wrote = m + 1;
      for (int j = 0; j < wrote; ++j) hist[(long long)b * L + p + j] = s_new[j];
    }
    if ((mode & 4) && m != 0) pos[b] = p + m;
    s_at[0] = p;
    s_at[1] = wrote;
    s_at[2] = (mode & 4) ? p + m : p;
  }
  __syncthreads();
  if (!(mode & 8)) return;
  const int p0 = s_at[0], wrote = s_at[1], pp = s_at[2];
  if (pp < 0 || pp >= L) {
    if (tid < K) out[b * K + tid] = 0;
    return;
  }
  const int* row = hist + (long long)b * L;
  auto H = [&](int i) { return i >= p0 && i < p0 + wrote ? s_new[i - p0] : row[i]; };   // 0 <= i <= pp
  const int pend = H(pp);
  const int nmax = min(3, pp);
  const int s1 = nmax >= 2 ? H(pp - 1) : 0, s2 = nmax >= 3 ? H(pp - 2) : 0;
  int best = -1;
  for (int t = tid; t < pp; t += 256) {
    if (H(t) != pend) continue;
    int ml = 1;
    if (nmax >= 2 && t >= 1 && H(t - 1) == s1) ml = (nmax >= 3 && t >= 2 && H(t - 2) == s2) ? 3 : 2;
    best = max(best, (ml << 28) | t);   // t < L <= 2^28
  }
  s_best[tid] = best;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) s_best[tid] = max(s_best[tid], s_best[tid + w]);
    __syncthreads();
  }
  if (tid < K) {
    const int key = s_best[0];
    const int t = key & ((1 << 28) - 1);
    out[b * K + tid] = (tid == 0 || key < 0 || t + tid > pp) ? pend : H(t + tid);
  }
}

// ------------------------------------------------------------------ sampling (temperature, top-k, top-p)
// u32 key of a logit, ordered as the floats are (-0 and +0, equal as floats, share a key)
__device__ __forceinline__ unsigned ord_key(float v) {
  if (v == 0.f) v = 0.f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = __umulhi(0xD2511F53u, c.x), l0 = 0xD2511F53u * c.x;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c.z), l1 = 0xCD9E8D57u * c.z;
    c = uint4{h1 ^ c.y ^ k0, l1, h0 ^ c.w ^ k1, l0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// One token per row drawn from softmax(x / T) restricted by top-k, then top-p
// (ctl = [T bits, top_k, top_p bits, seed], read here: one captured graph serves
// every request; all zero = greedy, exactly argmax_kernel's result).  One
// workgroup per row; the first pass copies the row (as fp32) into LDS where it
// fits (lds_row: 128 KB at vocab 32000 of the CU's 160 KB) and the later passes
// read it there (top-k with top-p makes 13 of them); a longer row, or any row
// where a workgroup's LDS limit is 64 KB, is re-read from L2:
//  1. the row maximum m and its index (am_better's rules);
//  2. top-k: the k-th largest logit by radix select on ord_key, 8-bit digits, an
//     integer LDS histogram per digit (ties at the k-th value all stay);
//  3. top-p: the smallest key whose mass of larger kept logits is < p Z, by a
//     descent over the same keys, 4-bit digits: 16 register sums per thread,
//     reduced by wave shuffles and then over the waves in wave order (no float
//     atomics: the sums, and so the token, repeat bit for bit);
//  4. the draw, Gumbel-max: score = (x - m) / T - log(-log(u)), u from word i & 3
//     of Philox4x32-10 at key (seed, row), counter (i >> 2, pos[row], 0, 0) -- the
//     position BEFORE this launch's pos_n advance -- the largest score wins, the
//     lower index on a tie.
template <int NT>
__global__ __launch_bounds__(NT) void sample_kernel(const void* __restrict__ x, int bf, int rows, int L, int ldx,
                                                    int* __restrict__ out, int* __restrict__ pos, int pos_n,
                                                    const int* __restrict__ ctl, int lds_row) {
  constexpr int NW = NT / 64;
  static_assert(NT >= 256, "the histogram scan takes 256 threads");
  extern __shared__ float rowc[];   // lds_row: the row, L floats
  __shared__ float sv[NW];
  __shared__ int si[NW];
  __shared__ float s_m;
  __shared__ int s_i, s_p;
  __shared__ int hist[256];
  __shared__ int wsum[4];
  __shared__ int s_d, s_k;
  __shared__ float part[NW][16];
  __shared__ float tot[16];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long long base = (long long)row * ldx;
  const float T = __int_as_float(ctl[0]), top_p = __int_as_float(ctl[2]);
  const int top_k = ctl[1];
  const unsigned seed = (unsigned)ctl[3];
  lds_row = lds_row && T > 0.f;   // greedy makes one pass
  // every lane of a wave makes the same trips (f sees in = j < L): f may vote across the wave
  // 8 loads in flight per thread
  auto walk = [&](auto&& f, bool first = false) {
    for (int b = wid * 64; b < L; b += 8 * NT) {
      float v[8];
      if (lds_row && !first) {   // the choice outside the batch: its loads issue together
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = b + u * NT + lane;
          const float r = rowc[j < L ? j : L - 1];
          v[u] = j < L ? r : -INFINITY;
        }
      } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = b + u * NT + lane;
          v[u] = j < L ? ldf(x, base + j, bf) : -INFINITY;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = b + u * NT + lane;
        f(v[u], j, j < L);
      }
    }
  };
  // (value, index) of the workgroup's best under `better`, in thread 0
  auto best_of = [&](float& best, int& bi, auto&& better) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ob, oi, best, bi)) {
        best = ob;
        bi = oi;
      }
    }
    if (lane == 0) {
      sv[wid] = best;
      si[wid] = bi;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < NW; ++w)
        if (better(sv[w], si[w], best, bi)) {
          best = sv[w];
          bi = si[w];
        }
  };

  // 1. the maximum
  float best = -INFINITY;
  int bi = INT_MAX;
  walk([&](float v, int j, bool in) {
    if (in && lds_row) rowc[j] = v;
    if (in && am_better(v, j, best, bi)) {
      best = v;
      bi = j;
    }
  }, true);
  best_of(best, bi, [](float bv, int bj, float av, int aj) { return am_better(bv, bj, av, aj); });
  if (tid == 0) {
    s_m = best;
    s_i = bi >= L ? 0 : bi;                  // an all -inf row: index 0
    s_p = pos != nullptr ? pos[row] : 0;     // the counter before this launch's advance (written below, by this thread)
  }
  __syncthreads();
  const float m = s_m;
  const int p0 = s_p;
  if (!(T > 0.f) || !(fabsf(m) < INFINITY)) {   // greedy; a NaN or infinite maximum
    if (tid == 0) {
      out[row] = s_i;
      if (pos != nullptr) pos[row] = p0 + pos_n;
    }
    return;
  }

  // 2. top-k: kept iff ord_key >= thr
  unsigned thr = 0;
  if (top_k > 0 && top_k < L) {
    unsigned prefix = 0;
    int kr = top_k;   // the kr-th largest of the keys under the prefix
    for (int r = 0; r < 4; ++r) {
      const int shift = 24 - 8 * r;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      walk([&](float v, int j, bool in) {
        const unsigned key = ord_key(v);
        const int d = (int)((key >> shift) & 255u);
        if (r == 0) {
          // logits share a few top bytes: one add per distinct digit of the wave, not 64
          // serialised ones on the same counter (still the dearest pass: docs/kernels.md)
          unsigned long long act = __ballot(in);
          while (act) {
            const int ld = __ffsll((long long)act) - 1;
            const int dl = __builtin_amdgcn_readlane(d, ld);   // ld is wave-uniform: no trip through LDS
            const unsigned long long same = __ballot(in && d == dl);
            if (lane == ld) atomicAdd(&hist[dl], __popcll(same));
            act &= ~same;
          }
        } else if (in && (key >> (shift + 8)) == prefix) {
          atomicAdd(&hist[d], 1);
        }
      });
      __syncthreads();
      // s = keys of digit >= tid: thread tid, whose digit the kr-th largest has, says so
      int h = 0, s = 0;
      if (tid < 256) {
        h = s = hist[tid];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_down(s, o, 64);
          if (lane + o < 64) s += t;
        }
        if (lane == 0) wsum[wid] = s;
      }
      __syncthreads();
      if (tid < 256) {
        for (int w = wid + 1; w < 4; ++w) s += wsum[w];
        if (s - h < kr && s >= kr) {
          s_d = tid;
          s_k = kr - (s - h);
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | (unsigned)s_d;
      kr = s_k;
    }
    thr = prefix;
  }

  // 3. top-p over the top-k set: kept iff ord_key >= the smallest key t with mass(key > t) < p Z
  if (top_p > 0.f && top_p < 1.f) {
    unsigned prefix = 0;
    float above = 0.f, pz = 0.f;   // mass of the keys over the prefix's range
    for (int r = 0; r < 8; ++r) {
      const int shift = 28 - 4 * r;
      float a[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) a[q] = 0.f;
      walk([&](float v, int j, bool in) {
        const unsigned key = ord_key(v);
        if (in && key >= thr && (r == 0 || (key >> (shift + 4)) == prefix)) {
          const float w = expf((v - m) / T);
          const int d = (int)((key >> shift) & 15u);
#pragma unroll
          for (int q = 0; q < 16; ++q) a[q] += d == q ? w : 0.f;
        }
      });
      // lanes trade halves of the 16 sums four times (8 + 4 + 2 + 1 shuffles): each then holds
      // one digit's sum over its 16 lanes; two more steps give the wave's
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int w = 8 >> st;
        const bool hi = (lane >> st) & 1;
#pragma unroll
        for (int q = 0; q < w; ++q) {
          const float send = hi ? a[q] : a[q + w];
          const float keep = hi ? a[q + w] : a[q];
          a[q] = keep + __shfl_xor(send, 1 << st, 64);
        }
      }
      a[0] += __shfl_xor(a[0], 16, 64);
      a[0] += __shfl_xor(a[0], 32, 64);
      if (lane < 16) part[wid][((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3)] = a[0];
      __syncthreads();
      if (tid < 16) {
        float t = 0.f;
        for (int w = 0; w < NW; ++w) t += part[w][tid];   // in wave order
        tot[tid] = t;
      }
      __syncthreads();
      float t[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) t[q] = tot[q];
      if (r == 0) {
        float Z = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) Z += t[q];
        pz = top_p * Z;
      }
      // the lowest digit whose keys still have less than p Z above them (the top one always has)
      int d0 = 15;
      float g = above, g0 = above;
      bool on = true;
#pragma unroll
      for (int d = 15; d >= 0; --d) {
        on = on && g < pz;
        d0 = on ? d : d0;
        g0 = on ? g : g0;
        g += t[d];
      }
      prefix = (prefix << 4) | (unsigned)d0;
      above = g0;
    }
    thr = prefix > thr ? prefix : thr;
  }

  // 4. the draw: 4 consecutive candidates share one Philox call
  best = -INFINITY;
  bi = INT_MAX;
  for (int g = tid; g < (L + 3) / 4; g += NT) {
    float v[4];
    bool keep[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = 4 * g + u;
      v[u] = j >= L ? -INFINITY : lds_row ? rowc[j] : ldf(x, base + j, bf);
      keep[u] = j < L && ord_key(v[u]) >= thr;
    }
    if (!(keep[0] || keep[1] || keep[2] || keep[3])) continue;
    const uint4 rnd = philox4x32_10(uint4{(unsigned)g, (unsigned)p0, 0u, 0u}, seed, (unsigned)row);
    const unsigned word[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float un = ((float)(word[u] >> 9) + 0.5f) * 1.1920928955078125e-07f;   // 2^-23: exact, in (0, 1)
      const float sc = (v[u] - m) / T - logf(-logf(un));
      const int j = 4 * g + u;
      if (keep[u] && (sc > best || (sc == best && j < bi))) {
        best = sc;
        bi = j;
      }
    }
  }
  best_of(best, bi, [](float bv, int bj, float av, int aj) { return bv > av || (bv == av && bj < aj); });
  if (tid == 0) {
    out[row] = bi >= L ? s_i : bi;
    if (pos != nullptr) pos[row] = p0 + pos_n;
  }
}

// ------------------------------------------------------------------ GEMV (M <= 8)
// x given as the decode attention's split partials (ws != null): x row m = sequence m's
// single query token, x[m][h * D + d] combined from the NS splits of (m, h / G) exactly as
// attn_decode_combine_kernel does -- the combine launch folded into the O-projection
struct Parts {
  const float* ws = nullptr;
  int NS = 0, R = 0, G = 0, Hkv = 0, D = 0;
};

__device__ __forceinline__ float4 parts_x4(const Parts& pt, int m, int k) {
  const int h = k / pt.D, d = k % pt.D, kvh = h / pt.G, r = h % pt.G;  // r = g (one query token)
  const int bk = m * pt.Hkv + kvh;
  const long long row = (long long)(pt.D + 2);
  float M = -INFINITY;
  for (int s = 0; s < pt.NS; ++s) {
    const float* p = pt.ws + ((long long)(bk * pt.NS + s) * pt.R + r) * row;
    if (p[pt.D + 1] > 0.f) M = fmaxf(M, p[pt.D]);
  }
  float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, den = 0.f;
  for (int s = 0; s < pt.NS; ++s) {
    const float* p = pt.ws + ((long long)(bk * pt.NS + s) * pt.R + r) * row;
    if (p[pt.D + 1] > 0.f) {
      const float w = __expf(p[pt.D] - M);
      n0 = fmaf(w, p[d], n0);
      n1 = fmaf(w, p[d + 1], n1);
      n2 = fmaf(w, p[d + 2], n2);
      n3 = fmaf(w, p[d + 3], n3);
      den = fmaf(w, p[pt.D + 1], den);
    }
  }
  return den > 0.f ? float4{n0 / den, n1 / den, n2 / den, n3 / den} : float4{0.f, 0.f, 0.f, 0.f};
}

// four x values of row m at column k as a GEMV stages them: read, or combined from the partials
__device__ __forceinline__ float4 gemv_x4(const Parts& pt, const void* x, int xbf, int ldx, int m, int k) {
  return pt.ws ? parts_x4(pt, m, k) : ld4(x, (long long)m * ldx + k, xbf);
}

// The adapter operand of a GEMV (the LoRA expand): output (m, n) gets + sum_j B[a_m - 1][n][j] t[m][j]
// before bias, activation, GLU or residual, with a_m = sel[m / rps]; rows whose a_m is outside [1, n]
// (0: the base model) skip the sum and are the plain kernel's bit for bit.  t [M][R] comes from
// nos_lora_shrink; B [n][N][R] has the adapter stride bsb and the row stride ldb.
struct Lora {
  const float* t = nullptr;
  const float* B = nullptr;
  const int* sel = nullptr;
  long long bsb = 0;
  int ldb = 0, R = 0, n = 0, rps = 1;
};
constexpr int LORA_MAX_R = 64;   // a lane per j: the R-long sum is one wave reduction
template <bool L>
struct LoraArg {
  int none = 0;
};
template <>
struct LoraArg<true> {
  Lora lo;
};
// t beside x in LDS (nothing in the plain instantiations)
template <bool L, int M>
struct LoraLds {};
template <int M>
struct LoraLds<true, M> {
  float t[M * LORA_MAX_R];
};

template <int M>
__device__ __forceinline__ void lora_stage(LoraLds<true, M>& ll, const Lora& lo, int tid) {
  for (int e = tid; e < M * lo.R; e += 256) ll.t[e] = lo.t[e];
}

// the rows' adapters (0: none, the base model), read at the kernel's start: wave-uniform registers
template <int M>
__device__ __forceinline__ void lora_rows(const Lora& lo, int (&am)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int a = lo.sel[m / lo.rps];
    am[m] = (a >= 1 && a <= lo.n) ? a : 0;
  }
}

// lane j's B[a - 1][n][j] of the delta of (a row with adapter a, weight row n): it depends on sel and
// n alone, so it is issued with the weight loads (the first group's with the weight prefetch, ahead
// of the x staging); times t[m][j] it is summed over the wave after the main product
__device__ __forceinline__ float lora_b(const Lora& lo, int a, int n, int lane) {
  return (a != 0 && lane < lo.R) ? lo.B[(long long)(a - 1) * lo.bsb + (long long)n * lo.ldb + lane] : 0.f;
}

// the scaled product v of (m, a weight row) plus the row's summed adapter delta d; a base row adds
// nothing (the plain kernel's bits), and the plain instantiations return v
template <bool L>
__device__ __forceinline__ float lora_add(float v, int a, float d) {
  if constexpr (L) {
    if (a != 0) v += d;
  }
  return v;
}

// one finished output (m, n) of a GEMV: v = the scaled product; bias in bbf's dtype, y / R in xbf's
__device__ __forceinline__ void gemv_finish(float v, int m, int n, int epi, const void* bias, int bbf, const void* res,
                                            int ldr, void* y, int ldy, int xbf) {
  if (epi & EPI_BIAS) v += ldf(bias, n, bbf);
  if (epi & EPI_GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  if (epi & EPI_RELU) v = fmaxf(v, 0.f);
  if (epi & EPI_SILU) v = v / (1.f + __expf(-v));
  if (epi & EPI_RESID) v += ldf(res, (long long)m * ldr + n, xbf);
  stf(y, (long long)m * ldy + n, v, xbf);
}

// EPI_GLU: output (m, n) = silu(gate) * up of the scaled products g (row n) and u (row n + Nh)
__device__ __forceinline__ void gemv_finish_glu(float g, float u, int m, int n, int Nh, int epi, const void* bias,
                                                int bbf, void* y, int ldy, int xbf) {
  if (epi & EPI_BIAS) {
    g += ldf(bias, n, bbf);
    u += ldf(bias, n + Nh, bbf);
  }
  stf(y, (long long)m * ldy + n, g / (1.f + __expf(-g)) * u, xbf);
}

template <int M, int WBF, int KU, bool LORA>
__global__ __launch_bounds__(256) void gemv_kernel(const void* __restrict__ x, int xbf, int ldx,
                                                   const void* __restrict__ w, int /*wbf = WBF*/, int ldw,
                                                   const void* __restrict__ bias, const void* __restrict__ res,
                                                   int ldr, void* __restrict__ y, int ldy, int N, int K, int epi,
                                                   float rms_eps, Parts pt, LoraArg<LORA> la) {
  constexpr int wbf = WBF;  // the weight dtype fixed at compile time: no per-load dtype branch
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [M][K] fp32
  __shared__ float rsc[M];
  __shared__ LoraLds<LORA, M> ll;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool glu = (epi & EPI_GLU) != 0;
  const int Nh = N / 2;                                          // GLU: output columns
  const int ngrp = glu ? (Nh + 3) / 4 : (N + 7) / 8;             // 8 columns per pass: 4 waves x 2
  // the weight rows (two per wave) of column group grp: GLU pairs gate n0 with up n0 + Nh
  auto rows_of = [&](int grp, int& n0, long long& w0, long long& w1) {
    n0 = glu ? grp * 4 + wid : grp * 8 + wid * 2;
    const int nc0 = glu ? min(n0, Nh - 1) : min(n0, N - 1);
    const int nc1 = glu ? min(n0, Nh - 1) + Nh : min(n0 + 1, N - 1);
    w0 = (long long)nc0 * ldw;
    w1 = (long long)nc1 * ldw;
  };
  auto load_chunk = [&](long long w0, long long w1, int k0, uint4 (&a)[KU], uint4 (&c4)[KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = k0 + 256 * u;
      a[u] = k < K ? ld4raw(w, w0 + k, wbf) : uint4{0u, 0u, 0u, 0u};
      c4[u] = k < K ? ld4raw(w, w1 + k, wbf) : uint4{0u, 0u, 0u, 0u};
    }
  };
  // the first group's first K chunk of weights in flight while x is staged and normalised:
  // the weights do not depend on x, and the two memory latencies were back to back
  uint4 pa[KU], pc[KU];
  if ((int)blockIdx.x < ngrp) {
    int n0;
    long long w0, w1;
    rows_of(blockIdx.x, n0, w0, w1);
    load_chunk(w0, w1, lane * 4, pa, pc);
  }
  [[maybe_unused]] int am[M];        // LORA: the rows' adapters
  [[maybe_unused]] float pb[2][M];   // LORA: the first group's B values, in flight with its weights
  // LORA: the weight rows (n0's pair) the delta of column group n0 reads, as rows_of clamps them
  auto lora_rows_of = [&](int n0, int (&nr)[2]) {
    nr[0] = glu ? min(n0, Nh - 1) : min(n0, N - 1);
    nr[1] = glu ? min(n0, Nh - 1) + Nh : min(n0 + 1, N - 1);
  };
  if constexpr (LORA) {
    lora_rows<M>(la.lo, am);
    if ((int)blockIdx.x < ngrp) {
      int nr[2];
      lora_rows_of(glu ? blockIdx.x * 4 + wid : blockIdx.x * 8 + wid * 2, nr);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) pb[c][m] = lora_b(la.lo, am[m], nr[c], lane);
    }
  }
  for (int e = tid * 4; e < M * K; e += 1024) {
    const int m = e / K, k = e % K;
    *reinterpret_cast<float4*>(&xs[e]) = gemv_x4(pt, x, xbf, ldx, m, k);
  }
  if constexpr (LORA) lora_stage<M>(ll, la.lo, tid);
  __syncthreads();
  if (rms_eps > 0.f) {  // RMSNorm of each row, gamma folded into W
    for (int m = wid; m < M; m += 4) {
      float q = 0.f;
      for (int k = lane; k < K; k += 64) q = fmaf(xs[m * K + k], xs[m * K + k], q);
      q = nos::wave_sum(q);
      if (lane == 0) rsc[m] = rsqrtf(q / (float)K + rms_eps);
    }
  } else if (tid < M) {
    rsc[tid] = 1.f;
  }
  __syncthreads();
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    int n0;
    long long w0, w1;
    rows_of(grp, n0, w0, w1);
    float acc[2][M];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = 0.f;
    float dl[2][M] = {};   // LORA: the adapter delta of (m, row c), a term per lane until it is summed
    if constexpr (LORA) {
      int nr[2];
      lora_rows_of(n0, nr);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const float b = grp == (int)blockIdx.x ? pb[c][m] : lora_b(la.lo, am[m], nr[c], lane);
          dl[c][m] = (am[m] != 0 && lane < la.lo.R) ? b * ll.t[m * la.lo.R + lane] : 0.f;
        }
    }
    // KU K steps' weight loads issued together (2 KU float4 in flight per lane): the
    // one-step loop waited a full memory latency per 256 columns of K; KU = 12 takes
    // K <= 3072 (a down projection) in one batch (the same summation order as KU = 4)
    for (int k0 = lane * 4; k0 < K; k0 += 256 * KU) {
      uint4 ra[KU], rc[KU];
      if (grp == (int)blockIdx.x && k0 == lane * 4) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          ra[u] = pa[u];
          rc[u] = pc[u];
        }
      } else {
        load_chunk(w0, w1, k0, ra, rc);
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int k = k0 + 256 * u;
        if (k < K) {
          const float4 a = cvt4(ra[u], wbf), c4 = cvt4(rc[u], wbf);
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const float4 xv = *reinterpret_cast<const float4*>(&xs[m * K + k]);
            acc[0][m] = fmaf(a.x, xv.x, fmaf(a.y, xv.y, fmaf(a.z, xv.z, fmaf(a.w, xv.w, acc[0][m]))));
            acc[1][m] = fmaf(c4.x, xv.x, fmaf(c4.y, xv.y, fmaf(c4.z, xv.z, fmaf(c4.w, xv.w, acc[1][m]))));
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = nos::wave_sum(acc[c][m]);
    if constexpr (LORA) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (am[m] != 0) dl[c][m] = nos::wave_sum(dl[c][m]);
    }
    if (glu) {  // lane m finishes output (m, n0): silu(gate) * up
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (lane == m && n0 < Nh)
          gemv_finish_glu(lora_add<LORA>(acc[0][m] * rsc[m], am[m], dl[0][m]),
                          lora_add<LORA>(acc[1][m] * rsc[m], am[m], dl[1][m]), m, n0, Nh, epi, bias, wbf, y, ldy, xbf);
      continue;
    }
    // lane (c * M + m) finishes output (m, n0 + c)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int n = n0 + c;
        if (lane == c * M + m && n < N)
          gemv_finish(lora_add<LORA>(acc[c][m] * rsc[m], am[m], dl[c][m]), m, n, epi, bias, wbf, res, ldr, y, ldy, xbf);
      }
  }
}

// ------------------------------------------------------------------ int8 weight-only GEMV (M <= 8)
// W = q [N, K] int8 with one fp32 scale per row (a storage format: the product is that of the
// dequantized fp32 weight): acc = sum_k x[m][k] (float)q[n][k] in fp32 FMAs, then
// y = act(acc * wscale[n] * rsc[m] + bias) + R.  A lane's 16-byte load is 16 consecutive k of one
// row, and a wave streams Q8_R rows (Q8_R x KU loads in flight per lane).  x sits in LDS as fp32,
// PERMUTED: in the natural layout a lane's four float4 of x for those 16 k lie 64 bytes from the
// next lane's, a 4-way conflict in every 16-lane group of ds_read_b128; here the four are, over the
// wave, four contiguous runs (16-byte lane stride, conflict-free):
//   k = 1024 b + 16 l + 4 j + e  ->  1024 b + 4 nl j + 4 l + e,  nl = min(64, (K - 1024 b) / 16)
// (nl: the lanes block b has work for; K % 16 == 0).  RMSNorm prologue: the statistics of the raw x
// rows are summed from the registers that stage them, and gamma (a pointer: per-row weight scales
// leave no room to fold it into W) multiplies x on its way into LDS.
constexpr int Q8_R = 4;   // weight rows per wave: 16 per workgroup pass (GLU: 8 gate + 8 up)

template <int M, int KU, bool LORA>
__global__ __launch_bounds__(256) void gemv_q8_kernel(const float* __restrict__ x, int ldx,
                                                      const signed char* __restrict__ w, int ldw,
                                                      const float* __restrict__ wscale,
                                                      const float* __restrict__ gamma, const float* __restrict__ bias,
                                                      const float* __restrict__ res, int ldr, float* __restrict__ y,
                                                      int ldy, int N, int K, int epi, float rms_eps, Parts pt,
                                                      LoraArg<LORA> la) {
  static_assert(Q8_R == 4, "the 4 x 4 word table below and the GLU pairing are written for four rows");
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [M][K] fp32, each row permuted as above
  __shared__ float rsc[M];
  __shared__ float sqp[4][M];   // the waves' sums of squares of each x row
  __shared__ LoraLds<LORA, M> ll;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool glu = (epi & EPI_GLU) != 0;
  const int Nh = N / 2;
  const int ngrp = glu ? (Nh + 7) / 8 : (N + 15) / 16;
  // the wave's Q8_R weight rows of column group grp; GLU: gates n0, n0 + 1, then their ups
  auto rows_of = [&](int grp, int& n0, long long (&wr)[Q8_R]) {
    n0 = glu ? grp * 8 + wid * 2 : grp * 16 + wid * Q8_R;
#pragma unroll
    for (int c = 0; c < Q8_R; ++c) {
      const int n = glu ? min(n0 + (c & 1), Nh - 1) + (c >> 1) * Nh : min(n0 + c, N - 1);
      wr[c] = (long long)n * ldw;
    }
  };
  auto load_chunk = [&](const long long (&wr)[Q8_R], int kb, uint4 (&a)[Q8_R][KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = kb + 1024 * u + lane * 16;
#pragma unroll
      for (int c = 0; c < Q8_R; ++c)
        a[c][u] = k < K ? *reinterpret_cast<const uint4*>(w + wr[c] + k) : uint4{0u, 0u, 0u, 0u};
    }
  };
  // the first group's first K chunk of weights in flight while x is staged (as gemv_kernel); later
  // groups' while the one before is computed
  uint4 pa[Q8_R][KU];
  if ((int)blockIdx.x < ngrp) {
    int n0;
    long long wr[Q8_R];
    rows_of(blockIdx.x, n0, wr);
    load_chunk(wr, 0, pa);
  }
  [[maybe_unused]] int am[M];           // LORA: the rows' adapters
  [[maybe_unused]] float pb[Q8_R][M];   // LORA: the first group's B values, in flight with its weights
  // LORA: the weight row of the wave's row c of column group n0, as rows_of clamps it
  auto lora_row_of = [&](int n0, int c) {
    return glu ? min(n0 + (c & 1), Nh - 1) + (c >> 1) * Nh : min(n0 + c, N - 1);
  };
  if constexpr (LORA) {
    lora_rows<M>(la.lo, am);
    if ((int)blockIdx.x < ngrp) {
      const int n0 = glu ? blockIdx.x * 8 + wid * 2 : blockIdx.x * 16 + wid * Q8_R;
#pragma unroll
      for (int c = 0; c < Q8_R; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) pb[c][m] = lora_b(la.lo, am[m], lora_row_of(n0, c), lane);
    }
  }
  float sq[M];
#pragma unroll
  for (int m = 0; m < M; ++m) sq[m] = 0.f;
  // p: the LDS position, its k from the permutation; a thread's loads go out four at a time (a
  // 2816-wide row is three per thread: one memory round trip, not three one after the other)
  constexpr int SU = 4;
  for (int p0 = tid * 4; p0 < M * K; p0 += 1024 * SU) {
    float4 v[SU], g[SU];
    int ms[SU];
#pragma unroll
    for (int s = 0; s < SU; ++s) {
      const int p = p0 + 1024 * s;
      if (p < M * K) {
        const int m = p / K, pk = p % K;
        const int b = pk >> 10, o = pk & 1023;
        const int nl = min(64, (K - (b << 10)) >> 4);
        const int k = (b << 10) + 16 * ((o % (4 * nl)) >> 2) + 4 * (o / (4 * nl));
        ms[s] = m;
        v[s] = gemv_x4(pt, x, 0, ldx, m, k);
        g[s] = gamma != nullptr ? *reinterpret_cast<const float4*>(gamma + k) : float4{1.f, 1.f, 1.f, 1.f};
      }
    }
#pragma unroll
    for (int s = 0; s < SU; ++s) {
      const int p = p0 + 1024 * s;
      if (p < M * K) {
        float4 t = v[s];
        if (rms_eps > 0.f) {
          const float q = fmaf(t.x, t.x, fmaf(t.y, t.y, fmaf(t.z, t.z, t.w * t.w)));
#pragma unroll
          for (int mm = 0; mm < M; ++mm) sq[mm] += mm == ms[s] ? q : 0.f;
          t = float4{t.x * g[s].x, t.y * g[s].y, t.z * g[s].z, t.w * g[s].w};
        }
        *reinterpret_cast<float4*>(&xs[p]) = t;
      }
    }
  }
  if (rms_eps > 0.f) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float t = nos::wave_sum(sq[m]);
      if (lane == 0) sqp[wid][m] = t;
    }
  }
  if constexpr (LORA) lora_stage<M>(ll, la.lo, tid);
  __syncthreads();
  if (tid < M)
    rsc[tid] = rms_eps > 0.f
                   ? rsqrtf(((sqp[0][tid] + sqp[1][tid]) + (sqp[2][tid] + sqp[3][tid])) / (float)K + rms_eps)
                   : 1.f;
  __syncthreads();
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    int n0;
    long long wr[Q8_R];
    rows_of(grp, n0, wr);
    float acc[Q8_R][M];
#pragma unroll
    for (int c = 0; c < Q8_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = 0.f;
    float dl[Q8_R][M] = {};   // LORA: the adapter delta of (m, row c), a term per lane until it is summed
    if constexpr (LORA) {
#pragma unroll
      for (int c = 0; c < Q8_R; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const float b = grp == (int)blockIdx.x ? pb[c][m] : lora_b(la.lo, am[m], lora_row_of(n0, c), lane);
          dl[c][m] = (am[m] != 0 && lane < la.lo.R) ? b * ll.t[m * la.lo.R + lane] : 0.f;
        }
    }
    for (int kb = 0; kb < K; kb += 1024 * KU) {
      uint4 ra[Q8_R][KU];
      if (kb == 0) {   // prefetched; the workgroup's next group's first chunk goes out before this one's math
#pragma unroll
        for (int c = 0; c < Q8_R; ++c)
#pragma unroll
          for (int u = 0; u < KU; ++u) ra[c][u] = pa[c][u];
        if (grp + (int)gridDim.x < ngrp) {
          int nn;
          long long wn[Q8_R];
          rows_of(grp + gridDim.x, nn, wn);
          load_chunk(wn, 0, pa);
        }
      } else {
        load_chunk(wr, kb, ra);
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int k0 = kb + 1024 * u;               // block k0 / 1024 of the row
        if (k0 + lane * 16 < K) {
          const int nl = min(64, (K - k0) >> 4);
          const unsigned wd[Q8_R][4] = {{ra[0][u].x, ra[0][u].y, ra[0][u].z, ra[0][u].w},
                                        {ra[1][u].x, ra[1][u].y, ra[1][u].z, ra[1][u].w},
                                        {ra[2][u].x, ra[2][u].y, ra[2][u].z, ra[2][u].w},
                                        {ra[3][u].x, ra[3][u].y, ra[3][u].z, ra[3][u].w}};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float4 wf[Q8_R];
#pragma unroll
            for (int c = 0; c < Q8_R; ++c) wf[c] = q8_cvt4(wd[c][j]);
#pragma unroll
            for (int m = 0; m < M; ++m) {
              const float4 xv = *reinterpret_cast<const float4*>(&xs[m * K + k0 + 4 * nl * j + 4 * lane]);
#pragma unroll
              for (int c = 0; c < Q8_R; ++c)
                acc[c][m] = fmaf(wf[c].x, xv.x, fmaf(wf[c].y, xv.y, fmaf(wf[c].z, xv.z, fmaf(wf[c].w, xv.w, acc[c][m]))));
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < Q8_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = nos::wave_sum(acc[c][m]);
    if constexpr (LORA) {
#pragma unroll
      for (int c = 0; c < Q8_R; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m)
          if (am[m] != 0) dl[c][m] = nos::wave_sum(dl[c][m]);
    }
    if (glu) {  // lane (c * M + m), c < 2, finishes output (m, n0 + c) from gate row c and up row c + 2
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int n = n0 + c;
          if (lane == c * M + m && n < Nh)
            gemv_finish_glu(lora_add<LORA>(acc[c][m] * wscale[n] * rsc[m], am[m], dl[c][m]),
                            lora_add<LORA>(acc[c + 2][m] * wscale[n + Nh] * rsc[m], am[m], dl[c + 2][m]), m, n, Nh,
                            epi, bias, 0, y, ldy, 0);
        }
      continue;
    }
    // lane (c * M + m) finishes output (m, n0 + c)
#pragma unroll
    for (int c = 0; c < Q8_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int n = n0 + c;
        if (lane == c * M + m && n < N)
          gemv_finish(lora_add<LORA>(acc[c][m] * wscale[n] * rsc[m], am[m], dl[c][m]), m, n, epi, bias, 0, res, ldr, y,
                      ldy, 0);
      }
  }
}

// ------------------------------------------------------------------ MXFP4 weight-only GEMV (M <= 8)
// W = codes [N, K / 2] u8 (two E2M1 elements per byte, element 2 i in the low nibble) with one E8M0
// scale byte e per 32 consecutive k of a row (scales [N, K / 32] u8, 2 <= e <= 252): a storage
// format, the product is that of the dequantized fp32 weight elem x 2^(e - 127), every such value a
// normal fp32.  gfx950 converts a byte of two codes to two fp32 with the block scale as an operand
// (v_cvt_scalef32_pk_f32_fp4; the scale is the float with bits e << 23), so the FMAs run on the
// dequantized values and nothing is left for the epilogue.  NOS_MX4_CVT_PLAIN builds the same decode
// from integer operations instead (sign, 3-bit magnitude, one exact multiply by the scale).
__device__ __forceinline__ float mx4_scale(unsigned e) { return __uint_as_float(e << 23); }

#ifdef NOS_MX4_CVT_PLAIN
__device__ __forceinline__ float mx4_cvt1(unsigned c, float s) {
  const unsigned mag = c & 7u;   // 0, 0.5, then 1, 1.5, 2, 3, 4, 6 = the fp32 with bits (mag << 22) + (126 << 23)
  const float el = mag < 2u ? 0.5f * (float)mag : __uint_as_float((mag << 22) + (126u << 23));
  return __uint_as_float(__float_as_uint(el * s) | ((c & 8u) << 28));
}
#endif

// elements 2 B, 2 B + 1 of the eight in word v (byte B: low nibble first), times the scale s
template <int B>
__device__ __forceinline__ float2 mx4_cvt2(unsigned v, float s) {
#ifdef NOS_MX4_CVT_PLAIN
  return float2{mx4_cvt1(v >> (8 * B), s), mx4_cvt1(v >> (8 * B + 4), s)};
#else
  const auto r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, B);
  return float2{r[0], r[1]};
#endif
}

// elements 4 H .. 4 H + 3 of word v
template <int H>
__device__ __forceinline__ float4 mx4_cvt4(unsigned v, float s) {
  const float2 a = mx4_cvt2<2 * H>(v, s), b = mx4_cvt2<2 * H + 1>(v, s);
  return float4{a.x, a.y, b.x, b.y};
}

// A lane's load is LB bytes of one row: KL = 2 LB consecutive k.  LB = 16 is exactly one MX block
// (one scale byte per lane, row and load; a wave's are 64 consecutive bytes) and a wave load covers
// 2048 k; LB = 8 is half a block (two lanes share a scale byte), 1024 k per wave load, so that a
// 1024-wide row still has work for all 64 lanes.  x sits in LDS as fp32, permuted as for the int8
// GEMV with the lane's run of KL k in place of 16:
//   k = 64 KL b + KL l + 4 j + e  ->  64 KL b + 4 nl j + 4 l + e,  j < KL / 4,  nl = min(64, (K - 64 KL b) / KL)
// so that the wave's read of the j-th float4 of every lane is one contiguous run (16-byte lane
// stride: ds_read_b128 conflict-free, by the argument above gemv_q8_kernel).  K % 32 == 0.
constexpr int MX4_R = 4;   // weight rows per wave, as Q8_R

template <int LB>
struct Mx4Words;
template <>
struct Mx4Words<16> {
  using T = uint4;
  static __device__ __forceinline__ void get(const uint4& v, unsigned (&w)[4]) {
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
};
template <>
struct Mx4Words<8> {
  using T = uint2;
  static __device__ __forceinline__ void get(const uint2& v, unsigned (&w)[2]) { w[0] = v.x, w[1] = v.y; }
};

template <int M, int KU, int LB>
__global__ __launch_bounds__(256) void gemv_mx4_kernel(const float* __restrict__ x, int ldx,
                                                       const unsigned char* __restrict__ w, int ldw,
                                                       const unsigned char* __restrict__ wsc, int ldsc,
                                                       const float* __restrict__ gamma, const float* __restrict__ bias,
                                                       const float* __restrict__ res, int ldr, float* __restrict__ y,
                                                       int ldy, int N, int K, int epi, float rms_eps, Parts pt) {
  static_assert(MX4_R == 4, "the GLU pairing is written for four rows");
  static_assert(LB == 16 || LB == 8, "a lane loads one MX block or half of one");
  constexpr int KL = 2 * LB, BLK = 64 * KL, NW = LB / 4;   // k per lane and per wave load; words per lane load
  using Ld = typename Mx4Words<LB>::T;
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [M][K] fp32, each row permuted as above
  __shared__ float rsc[M];
  __shared__ float sqp[4][M];   // the waves' sums of squares of each x row
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool glu = (epi & EPI_GLU) != 0;
  const int Nh = N / 2;
  const int ngrp = glu ? (Nh + 7) / 8 : (N + 15) / 16;
  // the wave's MX4_R weight rows of column group grp; GLU: gates n0, n0 + 1, then their ups
  auto rows_of = [&](int grp, int& n0, int (&nr)[MX4_R]) {
    n0 = glu ? grp * 8 + wid * 2 : grp * 16 + wid * MX4_R;
#pragma unroll
    for (int c = 0; c < MX4_R; ++c) nr[c] = glu ? min(n0 + (c & 1), Nh - 1) + (c >> 1) * Nh : min(n0 + c, N - 1);
  };
  // codes and the block's scale byte; past K: zeros under the scale 1
  auto load_chunk = [&](const int (&nr)[MX4_R], int kb, Ld (&a)[MX4_R][KU], unsigned (&e)[MX4_R][KU]) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = kb + BLK * u + lane * KL;
#pragma unroll
      for (int c = 0; c < MX4_R; ++c) {
        a[c][u] = k < K ? *reinterpret_cast<const Ld*>(w + (long long)nr[c] * ldw + (k >> 1)) : Ld{};
        e[c][u] = k < K ? (unsigned)wsc[(long long)nr[c] * ldsc + (k >> 5)] : 127u;
      }
    }
  };
  // the first group's first K chunk of weights in flight while x is staged (as gemv_kernel); later
  // groups' while the one before is computed
  Ld pa[MX4_R][KU];
  unsigned pe[MX4_R][KU];
  if ((int)blockIdx.x < ngrp) {
    int n0, nr[MX4_R];
    rows_of(blockIdx.x, n0, nr);
    load_chunk(nr, 0, pa, pe);
  }
  float sq[M];
#pragma unroll
  for (int m = 0; m < M; ++m) sq[m] = 0.f;
  // p: the LDS position, its k from the permutation; a thread's loads go out four at a time
  constexpr int SU = 4;
  for (int p0 = tid * 4; p0 < M * K; p0 += 1024 * SU) {
    float4 v[SU], g[SU];
    int ms[SU];
#pragma unroll
    for (int s = 0; s < SU; ++s) {
      const int p = p0 + 1024 * s;
      if (p < M * K) {
        const int m = p / K, pk = p % K;
        const int b = pk / BLK, o = pk % BLK;
        const int nl = min(64, (K - b * BLK) / KL);
        const int k = b * BLK + KL * ((o % (4 * nl)) >> 2) + 4 * (o / (4 * nl));
        ms[s] = m;
        v[s] = gemv_x4(pt, x, 0, ldx, m, k);
        g[s] = gamma != nullptr ? *reinterpret_cast<const float4*>(gamma + k) : float4{1.f, 1.f, 1.f, 1.f};
      }
    }
#pragma unroll
    for (int s = 0; s < SU; ++s) {
      const int p = p0 + 1024 * s;
      if (p < M * K) {
        float4 t = v[s];
        if (rms_eps > 0.f) {
          const float q = fmaf(t.x, t.x, fmaf(t.y, t.y, fmaf(t.z, t.z, t.w * t.w)));
#pragma unroll
          for (int mm = 0; mm < M; ++mm) sq[mm] += mm == ms[s] ? q : 0.f;
          t = float4{t.x * g[s].x, t.y * g[s].y, t.z * g[s].z, t.w * g[s].w};
        }
        *reinterpret_cast<float4*>(&xs[p]) = t;
      }
    }
  }
  if (rms_eps > 0.f) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float t = nos::wave_sum(sq[m]);
      if (lane == 0) sqp[wid][m] = t;
    }
  }
  __syncthreads();
  if (tid < M)
    rsc[tid] = rms_eps > 0.f
                   ? rsqrtf(((sqp[0][tid] + sqp[1][tid]) + (sqp[2][tid] + sqp[3][tid])) / (float)K + rms_eps)
                   : 1.f;
  __syncthreads();
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    int n0, nr[MX4_R];
    rows_of(grp, n0, nr);
    float acc[MX4_R][M];
#pragma unroll
    for (int c = 0; c < MX4_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = 0.f;
    for (int kb = 0; kb < K; kb += BLK * KU) {
      Ld ra[MX4_R][KU];
      unsigned re[MX4_R][KU];
      if (kb == 0) {   // prefetched; the workgroup's next group's first chunk goes out before this one's math
#pragma unroll
        for (int c = 0; c < MX4_R; ++c)
#pragma unroll
          for (int u = 0; u < KU; ++u) {
            ra[c][u] = pa[c][u];
            re[c][u] = pe[c][u];
          }
        if (grp + (int)gridDim.x < ngrp) {
          int nn, nrn[MX4_R];
          rows_of(grp + gridDim.x, nn, nrn);
          load_chunk(nrn, 0, pa, pe);
        }
      } else {
        load_chunk(nr, kb, ra, re);
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int k0 = kb + BLK * u;               // block k0 / BLK of the row
        if (k0 + lane * KL < K) {
          const int nl = min(64, (K - k0) / KL);
          unsigned wd[MX4_R][NW];
          float sc[MX4_R];
#pragma unroll
          for (int c = 0; c < MX4_R; ++c) {
            Mx4Words<LB>::get(ra[c][u], wd[c]);
            sc[c] = mx4_scale(re[c][u]);
          }
#pragma unroll
          for (int j2 = 0; j2 < NW; ++j2) {        // a word: 8 k, two float4 of x
            float4 wlo[MX4_R], whi[MX4_R];
#pragma unroll
            for (int c = 0; c < MX4_R; ++c) {
              wlo[c] = mx4_cvt4<0>(wd[c][j2], sc[c]);
              whi[c] = mx4_cvt4<1>(wd[c][j2], sc[c]);
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
              const float* xr = &xs[m * K + k0 + 4 * lane];
              const float4 x0 = *reinterpret_cast<const float4*>(xr + 4 * nl * (2 * j2));
              const float4 x1 = *reinterpret_cast<const float4*>(xr + 4 * nl * (2 * j2 + 1));
#pragma unroll
              for (int c = 0; c < MX4_R; ++c) {
                acc[c][m] = fmaf(wlo[c].x, x0.x, fmaf(wlo[c].y, x0.y, fmaf(wlo[c].z, x0.z, fmaf(wlo[c].w, x0.w, acc[c][m]))));
                acc[c][m] = fmaf(whi[c].x, x1.x, fmaf(whi[c].y, x1.y, fmaf(whi[c].z, x1.z, fmaf(whi[c].w, x1.w, acc[c][m]))));
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < MX4_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) acc[c][m] = nos::wave_sum(acc[c][m]);
    if (glu) {  // lane (c * M + m), c < 2, finishes output (m, n0 + c) from gate row c and up row c + 2
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int n = n0 + c;
          if (lane == c * M + m && n < Nh)
            gemv_finish_glu(acc[c][m] * rsc[m], acc[c + 2][m] * rsc[m], m, n, Nh, epi, bias, 0, y, ldy, 0);
        }
      continue;
    }
    // lane (c * M + m) finishes output (m, n0 + c)
#pragma unroll
    for (int c = 0; c < MX4_R; ++c)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int n = n0 + c;
        if (lane == c * M + m && n < N) gemv_finish(acc[c][m] * rsc[m], m, n, epi, bias, 0, res, ldr, y, ldy, 0);
      }
  }
}

// ------------------------------------------------------------------ LoRA shrink (M <= 8)
// t[m][j] = sum_k A[a_m - 1][j][k] xn[m][k], a_m = sel[m / rps]: the low-rank activations the GEMV after
// it expands (Lora).  xn is the x that GEMV multiplies: read with its staging helper (gemv_x4: an
// O-projection's x combined from the decode partials in the same arithmetic) and, under an RMSNorm
// prologue, normalised with the row's statistic and gamma.  A workgroup per (m, four rows j of A), its
// four waves splitting K: x is read once for four 16-byte streams of A, a 1024-wide row is ONE load
// per lane and stream (a down projection's 2816: three, issued together), and the waves' partial
// sums meet in LDS.  A row whose a_m is outside [1, n] writes zeros and reads nothing.
__global__ __launch_bounds__(256) void lora_shrink_kernel(const float* __restrict__ x, int ldx,
                                                          const float* __restrict__ A, long long bsa, int lda,
                                                          const int* __restrict__ sel, int n, int rps,
                                                          const float* __restrict__ gamma, float rms_eps,
                                                          float* __restrict__ t, int M, int R, int K, Parts pt) {
  __shared__ float part[4][5];   // each wave's four partial dot products and its sum of squares
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nq = R / 4;
  const int m = blockIdx.x / nq, j0 = (blockIdx.x % nq) * 4;   // grid: M x R / 4 workgroups
  const int a = sel[m / rps];
  float* out = t + (long long)m * R + j0;
  if (a < 1 || a > n) {   // the whole workgroup: no barrier is left behind
    if (tid < 4) out[tid] = 0.f;
    return;
  }
  const float* Ar = A + (long long)(a - 1) * bsa + (long long)j0 * lda;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float q = 0.f;
#pragma unroll 3
  for (int k = tid * 4; k < K; k += 1024) {
    float4 av[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) av[c] = *reinterpret_cast<const float4*>(Ar + (long long)c * lda + k);
    float4 xv = gemv_x4(pt, x, 0, ldx, m, k);
    if (rms_eps > 0.f) {
      q = fmaf(xv.x, xv.x, fmaf(xv.y, xv.y, fmaf(xv.z, xv.z, fmaf(xv.w, xv.w, q))));
      if (gamma != nullptr) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + k);
        xv = float4{xv.x * g.x, xv.y * g.y, xv.z * g.z, xv.w * g.w};
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      acc[c] = fmaf(av[c].x, xv.x, fmaf(av[c].y, xv.y, fmaf(av[c].z, xv.z, fmaf(av[c].w, xv.w, acc[c]))));
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = nos::wave_sum(acc[c]);
  q = nos::wave_sum(q);
  if (lane == 0) {
    part[wid][0] = acc[0];
    part[wid][1] = acc[1];
    part[wid][2] = acc[2];
    part[wid][3] = acc[3];
    part[wid][4] = q;
  }
  __syncthreads();
  if (tid < 4) {
    const float v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    const float qs = (part[0][4] + part[1][4]) + (part[2][4] + part[3][4]);
    out[tid] = rms_eps > 0.f ? v * rsqrtf(qs / (float)K + rms_eps) : v;
  }
}

// ------------------------------------------------------------------ mixture of experts (rows <= 8)
// y[m] = sum_s w[m][s] W2[e] (silu(W13[e][:I] x') * (W13[e][I:] x')), e = idx[m][s]: the k experts row m's
// router chose, in three launches -- route (idx, w), glu (act [rows][k][I]) and down (y).  x' is the x
// the GEMVs multiply: under an RMSNorm prologue the row's statistic is computed here and gamma read
// through a pointer (no expert weight is ever copied or folded).  Every sum has a fixed order (no
// atomics), so a step is bit-reproducible.  An index read from idx is checked against [0, E) before
// it forms an address: a slot outside it reads no weight and contributes zero.
constexpr int MOE_MAX_E = 64;   // a lane per expert in the softmax and the arg-max rounds
constexpr int MOE_MAX_K = 8;

// Row xr [H] into LDS as the GEMV prologue leaves it (times gamma under rms_eps > 0); returns the
// factor the products over xs are scaled by (1 without a prologue).  Every thread of the workgroup
// calls it; xs is complete on return.
__device__ __forceinline__ float moe_stage_x(const float* __restrict__ xr, const float* __restrict__ gamma,
                                             float rms_eps, int H, float* __restrict__ xs, float (&red)[4]) {
  const int tid = threadIdx.x;
  float q = 0.f;
  for (int k = tid * 4; k < H; k += 1024) {
    float4 xv = *reinterpret_cast<const float4*>(xr + k);
    if (rms_eps > 0.f) {
      q = fmaf(xv.x, xv.x, fmaf(xv.y, xv.y, fmaf(xv.z, xv.z, fmaf(xv.w, xv.w, q))));
      if (gamma != nullptr) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + k);
        xv = float4{xv.x * g.x, xv.y * g.y, xv.z * g.z, xv.w * g.w};
      }
    }
    *reinterpret_cast<float4*>(xs + k) = xv;
  }
  q = nos::wave_sum(q);
  if ((tid & 63) == 0) red[tid >> 6] = q;
  __syncthreads();
  return rms_eps > 0.f ? rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + rms_eps) : 1.f;
}

__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, acc))));
}

// One workgroup per row: the E router logits (the waves share the experts, 16-byte loads of Wr), the
// softmax over all E in wave 0 (a lane per expert), k arg-max rounds (a tie goes to the lower index)
// and the renormalisation: idx [rows][k], w [rows][k] in descending order of p.
__global__ __launch_bounds__(256) void moe_route_kernel(const float* __restrict__ x, int ldx,
                                                        const float* __restrict__ Wr, int ldwr,
                                                        const float* __restrict__ gamma, float rms_eps,
                                                        int* __restrict__ idx, float* __restrict__ w, int E, int H,
                                                        int k) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [H]
  __shared__ float red[4];
  __shared__ float logit[MOE_MAX_E];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m = blockIdx.x;
  // a wave takes the experts e0 and e0 + 4 together, KU K steps of both in flight: at E = 8 and
  // H = 1024 the whole router is one batch of loads per lane, issued ahead of the x staging
  constexpr int KU = 4;
  const float4 zero4 = float4{0.f, 0.f, 0.f, 0.f};
  auto load_pair = [&](int e0, int k0, float4 (&a)[KU], float4 (&c)[KU]) {
    const bool two = e0 + 4 < E;
    const float* r0 = Wr + (long long)e0 * ldwr;
    const float* r1 = Wr + (long long)(two ? e0 + 4 : e0) * ldwr;
    const int H1 = two ? H : 0;   // a missing second expert: no lane loads (a bound, not a branch per load)
#pragma unroll
    for (int j = 0; j < KU; ++j) {
      const int kk = k0 + 256 * j;
      a[j] = kk < H ? *reinterpret_cast<const float4*>(r0 + kk) : zero4;
      c[j] = kk < H1 ? *reinterpret_cast<const float4*>(r1 + kk) : zero4;
    }
  };
  float4 pa[KU], pc[KU];
  if (wid < E) load_pair(wid, lane * 4, pa, pc);
  const float rsc = moe_stage_x(x + (long long)m * ldx, gamma, rms_eps, H, xs, red);
  for (int e0 = wid; e0 < E; e0 += 8) {
    float a0 = 0.f, a1 = 0.f;
    for (int k0 = lane * 4; k0 < H; k0 += 256 * KU) {
      float4 ra[KU], rc[KU];
      if (e0 == wid && k0 == lane * 4) {
#pragma unroll
        for (int j = 0; j < KU; ++j) {
          ra[j] = pa[j];
          rc[j] = pc[j];
        }
      } else {
        load_pair(e0, k0, ra, rc);
      }
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        const int kk = k0 + 256 * j;
        if (kk < H) {
          const float4 xv = *reinterpret_cast<const float4*>(xs + kk);
          a0 = dot4(ra[j], xv, a0);
          a1 = dot4(rc[j], xv, a1);
        }
      }
    }
    a0 = nos::wave_sum(a0);
    a1 = nos::wave_sum(a1);
    if (lane == 0) {
      logit[e0] = a0 * rsc;
      if (e0 + 4 < E) logit[e0 + 4] = a1 * rsc;
    }
  }
  __syncthreads();
  if (wid != 0) return;
  const float l = lane < E ? logit[lane] : -INFINITY;
  const float mx = nos::wave_max(l);
  const float ex = lane < E ? expf(l - mx) : 0.f;
  const float p = ex / nos::wave_sum(ex);
  float cand = lane < E ? p : -1.f;   // a chosen expert leaves the running (p >= 0 > -1)
  float tot = 0.f, my_p = 0.f;
  int my_i = 0;
  for (int s = 0; s < k; ++s) {
    float bv = cand;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == s) {
      my_p = bv;
      my_i = bi;
    }
    if (lane == bi) cand = -1.f;
    tot += bv;
  }
  if (lane < k) {
    idx[(long long)m * k + lane] = my_i;
    w[(long long)m * k + lane] = my_p / tot;
  }
}

// Grid (column tiles of I) x (rows x k): pair (m, s) streams the gate and up rows of its expert's W13
// against x'[m] (a wave per column: gate row n and up row I + n, as the GEMV's GLU epilogue pairs
// them) and writes act[m][s][n] = silu(g) * u.  A slot whose index is outside [0, E) writes zeros.
__global__ __launch_bounds__(256) void moe_glu_kernel(const float* __restrict__ x, int ldx,
                                                      const int* __restrict__ idx, const float* __restrict__ W13,
                                                      long long bs13, int ld13, const float* __restrict__ gamma,
                                                      float rms_eps, float* __restrict__ act, int E, int H, int I,
                                                      int k) {
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [H]
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int pair = blockIdx.y, m = pair / k;
  const int e = __builtin_amdgcn_readfirstlane(idx[pair]);
  float* out = act + (long long)pair * I;
  const int ngrp = (I + 3) / 4;
  if (e < 0 || e >= E) {   // the whole workgroup: no barrier is left behind
    for (int n = blockIdx.x * 256 + tid; n < I; n += gridDim.x * 256) out[n] = 0.f;
    return;
  }
  const float* We = W13 + (long long)e * bs13;
  constexpr int KU = 4;
  auto load_chunk = [&](const float* g, const float* u, int k0, float4 (&a)[KU], float4 (&c)[KU]) {
#pragma unroll
    for (int j = 0; j < KU; ++j) {
      const int kk = k0 + 256 * j;
      a[j] = kk < H ? *reinterpret_cast<const float4*>(g + kk) : float4{0.f, 0.f, 0.f, 0.f};
      c[j] = kk < H ? *reinterpret_cast<const float4*>(u + kk) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  // the first group's first chunk of weights in flight while x is staged (as the GEMV does)
  float4 pa[KU], pc[KU];
  if ((int)blockIdx.x < ngrp) {
    const int n = min((int)blockIdx.x * 4 + wid, I - 1);
    load_chunk(We + (long long)n * ld13, We + (long long)(I + n) * ld13, lane * 4, pa, pc);
  }
  const float rsc = moe_stage_x(x + (long long)m * ldx, gamma, rms_eps, H, xs, red);
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    const int n0 = grp * 4 + wid, n = min(n0, I - 1);
    const float* g = We + (long long)n * ld13;
    const float* u = We + (long long)(I + n) * ld13;
    float ag = 0.f, au = 0.f;
    for (int k0 = lane * 4; k0 < H; k0 += 256 * KU) {
      float4 ra[KU], rc[KU];
      if (grp == (int)blockIdx.x && k0 == lane * 4) {
#pragma unroll
        for (int j = 0; j < KU; ++j) {
          ra[j] = pa[j];
          rc[j] = pc[j];
        }
      } else {
        load_chunk(g, u, k0, ra, rc);
      }
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        const int kk = k0 + 256 * j;
        if (kk < H) {
          const float4 xv = *reinterpret_cast<const float4*>(xs + kk);
          ag = dot4(ra[j], xv, ag);
          au = dot4(rc[j], xv, au);
        }
      }
    }
    ag = nos::wave_sum(ag) * rsc;
    au = nos::wave_sum(au) * rsc;
    if (lane == 0 && n0 < I) out[n0] = ag / (1.f + __expf(-ag)) * au;
  }
}

// Grid (column tiles of H) x rows: out[m][n] = res[m][n] + sum_{s < k} w[m][s] (W2[e_s][n] . act[m][s]),
// a column per wave; a lane sums its slots' terms in the order 0 .. k - 1 and the wave sum closes
// the column.  act[m] (k x I floats) sits in LDS.
__global__ __launch_bounds__(256) void moe_down_kernel(const float* __restrict__ act, const int* __restrict__ idx,
                                                       const float* __restrict__ w, const float* __restrict__ W2,
                                                       long long bs2, int ld2, const float* __restrict__ res, int ldr,
                                                       float* __restrict__ y, int ldy, int E, int H, int I, int k) {
  extern __shared__ __attribute__((aligned(16))) float as[];   // [k][I]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m = blockIdx.y;
  const float* am = act + (long long)m * k * I;
  for (int e4 = tid * 4; e4 < k * I; e4 += 1024)
    *reinterpret_cast<float4*>(as + e4) = *reinterpret_cast<const float4*>(am + e4);
  __syncthreads();
  // a column per wave (H = 1024 at one row: 256 workgroups, one per CU), its slots two at a time with
  // KU K steps of both in flight: I = 1408 at k = 2 is ONE batch of loads per lane, as the dense
  // down projection's K = 2816 is
  const int ngrp = (H + 3) / 4;
  constexpr int KU = 6;
  const float4 zero4 = float4{0.f, 0.f, 0.f, 0.f};
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    const int n0 = grp * 4 + wid, r = min(n0, H - 1);
    float acc = 0.f;
    for (int s = 0; s < k; s += 2) {
      const bool two = s + 1 < k;
      const int e0 = __builtin_amdgcn_readfirstlane(idx[(long long)m * k + s]);
      const int e1 = two ? __builtin_amdgcn_readfirstlane(idx[(long long)m * k + s + 1]) : -1;
      const bool v0 = e0 >= 0 && e0 < E, v1 = e1 >= 0 && e1 < E;   // wave-uniform; checked before any address
      if (!v0 && !v1) continue;
      const float* p0 = v0 ? W2 + (long long)e0 * bs2 + (long long)r * ld2 : W2;
      const float* p1 = v1 ? W2 + (long long)e1 * bs2 + (long long)r * ld2 : W2;
      const float* a0 = as + s * I;
      const float* a1 = as + (v1 ? s + 1 : s) * I;
      const int I0 = v0 ? I : 0, I1 = v1 ? I : 0;   // an invalid slot: no lane loads or adds (a bound, not a branch per load)
      float d0 = 0.f, d1 = 0.f;
      for (int k0 = lane * 4; k0 < I; k0 += 256 * KU) {
        float4 ra[KU], rc[KU];
#pragma unroll
        for (int j = 0; j < KU; ++j) {
          const int kk = k0 + 256 * j;
          ra[j] = kk < I0 ? *reinterpret_cast<const float4*>(p0 + kk) : zero4;
          rc[j] = kk < I1 ? *reinterpret_cast<const float4*>(p1 + kk) : zero4;
        }
#pragma unroll
        for (int j = 0; j < KU; ++j) {
          const int kk = k0 + 256 * j;
          if (kk < I0) d0 = dot4(ra[j], *reinterpret_cast<const float4*>(a0 + kk), d0);
          if (kk < I1) d1 = dot4(rc[j], *reinterpret_cast<const float4*>(a1 + kk), d1);
        }
      }
      if (v0) acc = fmaf(w[(long long)m * k + s], d0, acc);       // slot order: s, then s + 1
      if (v1) acc = fmaf(w[(long long)m * k + s + 1], d1, acc);
    }
    acc = nos::wave_sum(acc);
    if (lane == 0 && n0 < H) {
      if (res != nullptr) acc += res[(long long)m * ldr + n0];
      y[(long long)m * ldy + n0] = acc;
    }
  }
}

// ------------------------------------------------------------------ quantized experts (rows <= 8)
// The glu and down launches over expert tensors stored as int8 rows (W13q [E, 2I, H] i8 with scales
// [E, 2I] fp32, W2q [E, H, I] i8 with scales [E, H]) or as MXFP4 (codes [E, 2I, H / 2] u8 with scale
// bytes [E, 2I, H / 32], codes [E, H, I / 2] with [E, H, I / 32]): storage formats, the products are
// those of the dequantized fp32 experts.  The route launch is moe_route_kernel, unchanged; idx is
// checked against [0, E) before it forms an address, as above, and an invalid slot reads neither a
// weight nor a scale.  A lane's load is KL consecutive k of one row -- 16 int8; one MX block (32 k, 16
// bytes) or, where the row is at most NOS_MX4_NARROW_K long, half of one (16 k, 8 bytes) -- and a
// wave load covers BLK = 64 KL k, as in gemv_q8_kernel / gemv_mx4_kernel.
//
// The vector the rows multiply (x' in glu, act[m][s] in down; K floats) sits in LDS PERMUTED, by the
// GEMVs' rule with KL in place of 16:
//   k = BLK b + KL l + 4 j + e  ->  BLK b + 4 nl j + 4 l + e,  j < KL / 4,  nl = min(64, (K - BLK b) / KL)
// (nl: the lanes wave load b has work for; K % KL == 0).  Why: lane l needs the KL / 4 float4
// k = BLK b + KL l + 4 j.  In the natural layout the j-th float4 of neighbouring lanes lie 4 KL bytes
// apart (64 or 128), so the 64 banks x 4 bytes serve only every 4th (8th) lane of a ds_read_b128
// group at once: a 4-way (8-way) conflict.  Permuted, the j-th float4 of lanes 0 .. nl - 1 are the
// one contiguous run [BLK b + 4 nl j, BLK b + 4 nl (j + 1)): a 16-byte lane stride, each group of
// lanes the hardware serves together covers every bank exactly once, and the run starts 16-byte
// aligned (BLK b, 4 nl j and, in down, the slot's offset s I are multiples of 4 floats).  The map is a
// bijection of [0, K): block b keeps its nl KL positions, and (j, l) -> 4 nl j + 4 l is onto them.
template <int KL>
__device__ __forceinline__ int moe_perm_k(int p, int K) {   // the k of LDS position p (p % 4 == 0)
  constexpr int BLK = 64 * KL;
  const int b = p / BLK, o = p % BLK;
  const int nl = min(64, (K - b * BLK) / KL);
  return b * BLK + KL * ((o % (4 * nl)) >> 2) + 4 * (o / (4 * nl));
}

// int8 rows: the FMAs run on (float)q, the row's scale multiplies the wave's sum afterwards
struct MoeQ8 {
  static constexpr int KL = 16, KD = 2;   // KD: wave loads per batch of the down kernel (I = 1408: one batch)
  using Ld = uint4;
  // expert e's row n: its bytes, and the pointer its scale is read through
  struct Row {
    const unsigned char* w;
    const float* s;
  };
  static __device__ __forceinline__ Row row(const unsigned char* W, long long bsw, int ldw, const void* S,
                                            long long bss, int, int e, int n) {
    return Row{W + (long long)e * bsw + (long long)n * ldw, static_cast<const float*>(S) + (long long)e * bss + n};
  }
  static __device__ __forceinline__ void load(const Row& r, int k, int K, Ld& a, unsigned& sc) {
    a = k < K ? *reinterpret_cast<const uint4*>(r.w + k) : uint4{0u, 0u, 0u, 0u};
    sc = 0u;
  }
  static __device__ __forceinline__ float scale(const Row& r) { return *r.s; }
  // acc[c] += row c's KL weights . the lane's KL values of the staged vector (xb: its first float4)
  template <int R>
  static __device__ __forceinline__ void dot(const Ld (&a)[R], const unsigned (&)[R], const float* xb, int nl,
                                             float (&acc)[R]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4 xv = *reinterpret_cast<const float4*>(xb + 4 * nl * j);
#pragma unroll
      for (int c = 0; c < R; ++c) {
        const unsigned wd = j == 0 ? a[c].x : j == 1 ? a[c].y : j == 2 ? a[c].z : a[c].w;
        acc[c] = dot4(q8_cvt4(wd), xv, acc[c]);
      }
    }
  }
};

// MXFP4 rows: the FMAs run on elem x 2^(e - 127) (mx4_cvt4: the hardware conversion, or the plain
// one under NOS_MX4_CVT_PLAIN); nothing is left for the epilogue
template <int LB>
struct MoeMx4 {
  static_assert(LB == 16 || LB == 8, "a lane loads one MX block or half of one");
  static constexpr int KL = 2 * LB, NW = LB / 4, KD = LB == 16 ? 1 : 2;
  using Ld = typename Mx4Words<LB>::T;
  struct Row {
    const unsigned char* w;
    const unsigned char* s;
  };
  static __device__ __forceinline__ Row row(const unsigned char* W, long long bsw, int ldw, const void* S,
                                            long long bss, int lds, int e, int n) {
    return Row{W + (long long)e * bsw + (long long)n * ldw,
               static_cast<const unsigned char*>(S) + (long long)e * bss + (long long)n * lds};
  }
  // codes and the block's scale byte; past K: zeros under the scale 1
  static __device__ __forceinline__ void load(const Row& r, int k, int K, Ld& a, unsigned& sc) {
    a = k < K ? *reinterpret_cast<const Ld*>(r.w + (k >> 1)) : Ld{};
    sc = k < K ? (unsigned)r.s[k >> 5] : 127u;
  }
  static __device__ __forceinline__ float scale(const Row&) { return 1.f; }
  template <int R>
  static __device__ __forceinline__ void dot(const Ld (&a)[R], const unsigned (&sc)[R], const float* xb, int nl,
                                             float (&acc)[R]) {
    unsigned wd[R][NW];
    float s[R];
#pragma unroll
    for (int c = 0; c < R; ++c) {
      Mx4Words<LB>::get(a[c], wd[c]);
      s[c] = mx4_scale(sc[c]);
    }
#pragma unroll
    for (int j2 = 0; j2 < NW; ++j2) {   // a word: 8 k, two float4 of the staged vector
      const float4 x0 = *reinterpret_cast<const float4*>(xb + 4 * nl * (2 * j2));
      const float4 x1 = *reinterpret_cast<const float4*>(xb + 4 * nl * (2 * j2 + 1));
#pragma unroll
      for (int c = 0; c < R; ++c) {
        acc[c] = dot4(mx4_cvt4<0>(wd[c][j2], s[c]), x0, acc[c]);
        acc[c] = dot4(mx4_cvt4<1>(wd[c][j2], s[c]), x1, acc[c]);
      }
    }
  }
};

// moe_stage_x into the permuted layout of lane runs of KL: xs complete on return, the factor returned
template <int KL>
__device__ __forceinline__ float moe_stage_xp(const float* __restrict__ xr, const float* __restrict__ gamma,
                                              float rms_eps, int H, float* __restrict__ xs, float (&red)[4]) {
  const int tid = threadIdx.x;
  float q = 0.f;
  for (int p = tid * 4; p < H; p += 1024) {
    const int k = moe_perm_k<KL>(p, H);
    float4 xv = *reinterpret_cast<const float4*>(xr + k);
    if (rms_eps > 0.f) {
      q = fmaf(xv.x, xv.x, fmaf(xv.y, xv.y, fmaf(xv.z, xv.z, fmaf(xv.w, xv.w, q))));
      if (gamma != nullptr) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + k);
        xv = float4{xv.x * g.x, xv.y * g.y, xv.z * g.z, xv.w * g.w};
      }
    }
    *reinterpret_cast<float4*>(xs + p) = xv;
  }
  q = nos::wave_sum(q);
  if ((tid & 63) == 0) red[tid >> 6] = q;
  __syncthreads();
  return rms_eps > 0.f ? rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + rms_eps) : 1.f;
}

// moe_glu_kernel over quantized rows.  Grid (column tiles of I) x (rows x k); a wave streams FOUR rows
// of its pair's expert -- the gates n0, n0 + 1 and their ups I + n0, I + n0 + 1, as the GEMVs' GLU form
// pairs them -- so a workgroup pass is 8 columns; the first group's first wave load goes out before x
// is staged, every later group's while the one before is computed.
template <class F>
__global__ __launch_bounds__(256) void moe_glu_quant_kernel(const float* __restrict__ x, int ldx,
                                                            const int* __restrict__ idx,
                                                            const unsigned char* __restrict__ W, long long bsw,
                                                            int ldw, const void* __restrict__ S, long long bss,
                                                            int lds, const float* __restrict__ gamma, float rms_eps,
                                                            float* __restrict__ act, int E, int H, int I, int k) {
  constexpr int KL = F::KL, BLK = 64 * KL, R = 4;
  using Ld = typename F::Ld;
  extern __shared__ __attribute__((aligned(16))) float xs[];   // [H], permuted as above
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int pair = blockIdx.y, m = pair / k;
  const int e = __builtin_amdgcn_readfirstlane(idx[pair]);
  float* out = act + (long long)pair * I;
  const int ngrp = (I + 7) / 8;
  if (e < 0 || e >= E) {   // the whole workgroup: no barrier is left behind, no weight or scale is read
    for (int n = blockIdx.x * 256 + tid; n < I; n += gridDim.x * 256) out[n] = 0.f;
    return;
  }
  auto rows_of = [&](int grp, int& n0, typename F::Row (&rw)[R]) {
    n0 = grp * 8 + wid * 2;
#pragma unroll
    for (int c = 0; c < R; ++c) rw[c] = F::row(W, bsw, ldw, S, bss, lds, e, min(n0 + (c & 1), I - 1) + (c >> 1) * I);
  };
  auto load_chunk = [&](const typename F::Row (&rw)[R], int kb, Ld (&a)[R], unsigned (&sc)[R]) {
#pragma unroll
    for (int c = 0; c < R; ++c) F::load(rw[c], kb + lane * KL, H, a[c], sc[c]);
  };
  Ld pa[R];
  unsigned pe[R];
  if ((int)blockIdx.x < ngrp) {
    int n0;
    typename F::Row rw[R];
    rows_of(blockIdx.x, n0, rw);
    load_chunk(rw, 0, pa, pe);
  }
  const float rsc = moe_stage_xp<KL>(x + (long long)m * ldx, gamma, rms_eps, H, xs, red);
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    int n0;
    typename F::Row rw[R];
    rows_of(grp, n0, rw);
    float acc[R] = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < H; kb += BLK) {
      Ld ra[R];
      unsigned re[R];
      if (kb == 0) {   // prefetched; the workgroup's next group's first load goes out before this one's math
#pragma unroll
        for (int c = 0; c < R; ++c) {
          ra[c] = pa[c];
          re[c] = pe[c];
        }
        if (grp + (int)gridDim.x < ngrp) {
          int nn;
          typename F::Row rn[R];
          rows_of(grp + gridDim.x, nn, rn);
          load_chunk(rn, 0, pa, pe);
        }
      } else {
        load_chunk(rw, kb, ra, re);
      }
      if (kb + lane * KL < H) F::template dot<R>(ra, re, xs + kb + 4 * lane, min(64, (H - kb) / KL), acc);
    }
#pragma unroll
    for (int c = 0; c < R; ++c) acc[c] = nos::wave_sum(acc[c]);
#pragma unroll
    for (int c = 0; c < 2; ++c) {   // lane c finishes column n0 + c from gate row c and up row c + 2
      const int n = n0 + c;
      if (lane == c && n < I) {
        const float ag = acc[c] * F::scale(rw[c]) * rsc, au = acc[c + 2] * F::scale(rw[c + 2]) * rsc;
        out[n] = ag / (1.f + __expf(-ag)) * au;
      }
    }
  }
}

// moe_down_kernel over quantized rows.  Grid (column tiles of H) x rows; a wave takes R columns (R = 2
// where that still fills the CUs, else 1; R = 4 with two slots in flight takes all 256 VGPRs) and walks its row's slots two at a time in the order
// 0 .. k - 1, KD wave loads of both slots and all R rows in flight; a lane folds w[m][s] (int8: times
// the row's scale s2[e_s][n]) into its running term per slot, and the wave sum closes the column: no
// atomics, a fixed order.  act[m] (k x I floats) sits in LDS, every slot permuted as above; the first
// group's first batch goes out before it is staged.
template <class F, int R>
__global__ __launch_bounds__(256) void moe_down_quant_kernel(const float* __restrict__ act,
                                                             const int* __restrict__ idx, const float* __restrict__ w,
                                                             const unsigned char* __restrict__ W, long long bsw,
                                                             int ldw, const void* __restrict__ S, long long bss,
                                                             int lds, const float* __restrict__ res, int ldr,
                                                             float* __restrict__ y, int ldy, int E, int H, int I,
                                                             int k) {
  constexpr int KL = F::KL, BLK = 64 * KL, KD = F::KD;
  using Ld = typename F::Ld;
  extern __shared__ __attribute__((aligned(16))) float as[];   // [k][I], each slot permuted as above
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m = blockIdx.y;
  const int ngrp = (H + 4 * R - 1) / (4 * R);
  // slots s, s + 1 of row m: the experts (-1: none, or outside [0, E): wave-uniform, checked before any address)
  auto slots_of = [&](int s, int& e0, int& e1) {
    e0 = __builtin_amdgcn_readfirstlane(idx[(long long)m * k + s]);
    e1 = s + 1 < k ? __builtin_amdgcn_readfirstlane(idx[(long long)m * k + s + 1]) : -1;
    if (e0 < 0 || e0 >= E) e0 = -1;
    if (e1 < 0 || e1 >= E) e1 = -1;
  };
  // a batch: KD wave loads from kb of the R rows of expert e (e < 0: no lane loads)
  auto load_batch = [&](int e, int n0, int kb, Ld (&a)[R][KD], unsigned (&sc)[R][KD]) {
    const int I0 = e >= 0 ? I : 0;   // a bound, not a branch per load
#pragma unroll
    for (int c = 0; c < R; ++c) {
      const typename F::Row rw = F::row(W, bsw, ldw, S, bss, lds, e >= 0 ? e : 0, min(n0 + c, H - 1));
#pragma unroll
      for (int u = 0; u < KD; ++u) F::load(rw, kb + BLK * u + lane * KL, I0, a[c][u], sc[c][u]);
    }
  };
  Ld pa0[R][KD], pa1[R][KD];
  unsigned pe0[R][KD], pe1[R][KD];
  if ((int)blockIdx.x < ngrp) {
    int e0, e1;
    slots_of(0, e0, e1);
    const int n0 = blockIdx.x * 4 * R + wid * R;
    load_batch(e0, n0, 0, pa0, pe0);
    load_batch(e1, n0, 0, pa1, pe1);
  }
  const float* am = act + (long long)m * k * I;
  for (int p = tid * 4; p < k * I; p += 1024) {
    const int s = p / I;   // I % 4 == 0: a float4 stays inside its slot
    *reinterpret_cast<float4*>(as + p) = *reinterpret_cast<const float4*>(am + s * I + moe_perm_k<KL>(p - s * I, I));
  }
  __syncthreads();
  for (int grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
    const int n0 = grp * 4 * R + wid * R;
    float acc[R];
#pragma unroll
    for (int c = 0; c < R; ++c) acc[c] = 0.f;
    for (int s = 0; s < k; s += 2) {
      int e0, e1;
      slots_of(s, e0, e1);
      if (e0 < 0 && e1 < 0) continue;
      float d0[R], d1[R];
#pragma unroll
      for (int c = 0; c < R; ++c) d0[c] = d1[c] = 0.f;
      for (int kb = 0; kb < I; kb += BLK * KD) {
        Ld ra[R][KD], rc[R][KD];
        unsigned re[R][KD], rf[R][KD];
        if (grp == (int)blockIdx.x && s == 0 && kb == 0) {
#pragma unroll
          for (int c = 0; c < R; ++c)
#pragma unroll
            for (int u = 0; u < KD; ++u) {
              ra[c][u] = pa0[c][u], re[c][u] = pe0[c][u];
              rc[c][u] = pa1[c][u], rf[c][u] = pe1[c][u];
            }
        } else {
          load_batch(e0, n0, kb, ra, re);
          load_batch(e1, n0, kb, rc, rf);
        }
#pragma unroll
        for (int u = 0; u < KD; ++u) {
          const int k0 = kb + BLK * u;
          if (k0 + lane * KL < I) {
            const int nl = min(64, (I - k0) / KL);
            Ld ta[R], tc[R];
            unsigned te[R], tf[R];
#pragma unroll
            for (int c = 0; c < R; ++c) {
              ta[c] = ra[c][u], te[c] = re[c][u];
              tc[c] = rc[c][u], tf[c] = rf[c][u];
            }
            if (e0 >= 0) F::template dot<R>(ta, te, as + s * I + k0 + 4 * lane, nl, d0);
            if (e1 >= 0) F::template dot<R>(tc, tf, as + (s + 1) * I + k0 + 4 * lane, nl, d1);
          }
        }
      }
      // slot order: s, then s + 1; the weights and scales of a valid slot only
#pragma unroll
      for (int c = 0; c < R; ++c) {
        const int n = min(n0 + c, H - 1);
        if (e0 >= 0)
          acc[c] = fmaf(w[(long long)m * k + s] * F::scale(F::row(W, bsw, ldw, S, bss, lds, e0, n)), d0[c], acc[c]);
        if (e1 >= 0)
          acc[c] = fmaf(w[(long long)m * k + s + 1] * F::scale(F::row(W, bsw, ldw, S, bss, lds, e1, n)), d1[c], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < R; ++c) acc[c] = nos::wave_sum(acc[c]);
#pragma unroll
    for (int c = 0; c < R; ++c) {
      const int n = n0 + c;
      if (lane == c && n < H) {
        float v = acc[c];
        if (res != nullptr) v += res[(long long)m * ldr + n];
        y[(long long)m * ldy + n] = v;
      }
    }
  }
}

// out [N, K] fp32 = (float)q * wscale[n], one rounding: 4 weights per thread (a 4-byte load, a 16-byte store)
__global__ __launch_bounds__(256) void dequant_q8_kernel(const signed char* __restrict__ w, int ldw,
                                                         const float* __restrict__ wscale, float* __restrict__ out,
                                                         int ldo, int N, int K) {
  const long long total = (long long)N * (K / 4);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / (K / 4)), k = (int)(i % (K / 4)) * 4;
    const float4 q = q8_cvt4(*reinterpret_cast<const unsigned*>(w + (long long)n * ldw + k));
    const float s = wscale[n];
    *reinterpret_cast<float4*>(out + (long long)n * ldo + k) = float4{q.x * s, q.y * s, q.z * s, q.w * s};
  }
}

// out [N, K] fp32 = elem x 2^(e - 127) of the MXFP4 weight, the GEMV's own conversion: 8 weights per
// thread (a 4-byte load of codes and the block's scale byte, two 16-byte stores)
__global__ __launch_bounds__(256) void dequant_mx4_kernel(const unsigned char* __restrict__ w, int ldw,
                                                          const unsigned char* __restrict__ wsc, int ldsc,
                                                          float* __restrict__ out, int ldo, int N, int K) {
  const long long total = (long long)N * (K / 8);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i / (K / 8)), k = (int)(i % (K / 8)) * 8;
    const unsigned v = *reinterpret_cast<const unsigned*>(w + (long long)n * ldw + (k >> 1));
    const float s = mx4_scale(wsc[(long long)n * ldsc + (k >> 5)]);
    float* o = out + (long long)n * ldo + k;
    *reinterpret_cast<float4*>(o) = mx4_cvt4<0>(v, s);
    *reinterpret_cast<float4*>(o + 4) = mx4_cvt4<1>(v, s);
  }
}

}  // namespace

// x2 / cache2 (optional, same shapes and dtypes): a second write in the same
// launch without rotation -- a layer's V beside its rotated K
NOS_API int nos_kv_write(const void* x, int xbf, int ldx, long long bsx, void* cache, int cbf, const int* pos,
                         const float* cos_t, const float* sin_t, int R, int B, int S, int H, int D, int L,
                         const void* x2, int ldx2, long long bsx2, void* cache2, hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || D <= 0 || (D % 2) || L <= 0 || S > L || ldx < H * D || !x || !cache || !pos ||
      (B > 1 && bsx < (long long)(S - 1) * ldx + H * D) || (xbf != 0 && xbf != 1) || (cbf != 0 && cbf != 1) ||
      ((cos_t == nullptr) != (sin_t == nullptr)) || (cos_t && R <= 0) || ((x2 == nullptr) != (cache2 == nullptr)) ||
      (x2 && (ldx2 < H * D || (B > 1 && bsx2 < (long long)(S - 1) * ldx2 + H * D))))
    return (int)hipErrorInvalidValue;
  const long long n = (long long)B * S * H * (D / 2);
  hipLaunchKernelGGL(kv_write_kernel, dim3((unsigned)((n + 255) / 256), x2 ? 2u : 1u), dim3(256), 0, stream, x, xbf,
                     ldx, bsx, cache, cbf, pos, cos_t, sin_t, R, B, S, H, D, L, KvPair{x2, ldx2, bsx2, cache2});
  return (int)hipGetLastError();
}

// the arguments of a ring cache of C slots at a step of S rows: window W >= 1, min(limit, W + S - 1) <= C
// <= limit (the step's rows and the first row's window fit), and the rotary tables cover every stored position
static bool ring_ok(int C, int S, int W, int limit, bool rope, int R) {
  return nos::ring_args_ok(C, S, W, limit, rope, R);   // kv_ring.h: shared with attention_h3g.hip
}

// nos_kv_write into ring caches [B, C, H, D] (kv_ring.h): the row of position p = pos[b] + s goes to slot
// p % C, rows at p < 0 or p >= limit are dropped; window: the attention's, for the size check only
NOS_API int nos_kv_write_ring(const void* x, int xbf, int ldx, long long bsx, void* cache, int cbf, const int* pos,
                              const float* cos_t, const float* sin_t, int R, int B, int S, int H, int D, int C,
                              const void* x2, int ldx2, long long bsx2, void* cache2, int window, int limit,
                              hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || D <= 0 || (D % 2) || C <= 0 || S > C || ldx < H * D || !x || !cache || !pos ||
      (B > 1 && bsx < (long long)(S - 1) * ldx + H * D) || (xbf != 0 && xbf != 1) || (cbf != 0 && cbf != 1) ||
      ((cos_t == nullptr) != (sin_t == nullptr)) || (cos_t && R <= 0) || ((x2 == nullptr) != (cache2 == nullptr)) ||
      (x2 && (ldx2 < H * D || (B > 1 && bsx2 < (long long)(S - 1) * ldx2 + H * D))) ||
      !ring_ok(C, S, window, limit, cos_t != nullptr, R))
    return (int)hipErrorInvalidValue;
  const long long n = (long long)B * S * H * (D / 2);
  hipLaunchKernelGGL(kv_write_ring_kernel, dim3((unsigned)((n + 255) / 256), x2 ? 2u : 1u), dim3(256), 0, stream, x,
                     xbf, ldx, bsx, cache, cbf, pos, cos_t, sin_t, R, B, S, H, D, C, KvPair{x2, ldx2, bsx2, cache2},
                     limit);
  return (int)hipGetLastError();
}

// nos_kv_write_q8 into int8 ring caches [B, C, H, D] with their row scales [B, C, H]
NOS_API int nos_kv_write_ring_q8(const float* x, int ldx, long long bsx, void* cache, float* scales, float* deq,
                                 const int* pos, const float* cos_t, const float* sin_t, int R, int B, int S, int H,
                                 int D, int C, const float* x2, int ldx2, long long bsx2, void* cache2,
                                 float* scales2, float* deq2, int window, int limit, hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || (D != 64 && D != 128) || C <= 0 || S > C || ldx < H * D || !x || !cache ||
      !scales || !pos || (B > 1 && bsx < (long long)(S - 1) * ldx + H * D) || ((uintptr_t)cache & 15) ||
      ((uintptr_t)scales & 3) || ((uintptr_t)x & 3) || ((uintptr_t)deq & 3) ||
      ((cos_t == nullptr) != (sin_t == nullptr)) || (cos_t && R <= 0) || ((x2 == nullptr) != (cache2 == nullptr)) ||
      ((x2 == nullptr) != (scales2 == nullptr)) || (!x2 && deq2) ||
      (x2 && (ldx2 < H * D || (B > 1 && bsx2 < (long long)(S - 1) * ldx2 + H * D) || ((uintptr_t)cache2 & 15) ||
              ((uintptr_t)scales2 & 3) || ((uintptr_t)x2 & 3) || ((uintptr_t)deq2 & 3))) ||
      !ring_ok(C, S, window, limit, cos_t != nullptr, R))
    return (int)hipErrorInvalidValue;
  const long long rows = (long long)B * S * H;
  const dim3 grid((unsigned)((rows + 3) / 4), x2 ? 2u : 1u);
  const KvPairQ8 v2{x2, ldx2, bsx2, static_cast<signed char*>(cache2), scales2, deq2};
  if (D == 64)
    hipLaunchKernelGGL(kv_write_q8_ring_kernel<64>, grid, dim3(256), 0, stream, x, ldx, bsx,
                       static_cast<signed char*>(cache), scales, deq, pos, cos_t, sin_t, R, B, S, H, C, v2, limit);
  else
    hipLaunchKernelGGL(kv_write_q8_ring_kernel<128>, grid, dim3(256), 0, stream, x, ldx, bsx,
                       static_cast<signed char*>(cache), scales, deq, pos, cos_t, sin_t, R, B, S, H, C, v2, limit);
  return (int)hipGetLastError();
}

// the slot and visibility arithmetic the ring kernels use (kv_ring.h), for tests on the host
NOS_API int nos_ring_slot(int p, int C, int limit) { return nos::ring_slot(p, C, limit); }
NOS_API int nos_ring_position(int s, int pmax, int C) { return nos::ring_position(s, pmax, C); }
NOS_API int nos_ring_visible(int s, int qpos, int pmax, int C, int W) { return nos::ring_visible(s, qpos, pmax, C, W); }
NOS_API int nos_ring_oldest(int qlo, int pmax, int C, int W) { return nos::ring_oldest(qlo, pmax, C, W); }
NOS_API int nos_ring_split_rows(int k0, int n, int lo, int hi, int C) { return nos::ring_split_rows(k0, n, lo, hi, C); }

// nos_kv_write into int8 caches: x fp32, cache [B, L, H, D] int8 (16-byte aligned) with its row scales
// [B, L, H] fp32, D = 64 / 128; deq (or null): [B, S, H, D] fp32 contiguous, the rows as the cache holds
// them.  x2 / cache2 / scales2 / deq2: the unrotated second write of the launch (V).
NOS_API int nos_kv_write_q8(const float* x, int ldx, long long bsx, void* cache, float* scales, float* deq,
                            const int* pos, const float* cos_t, const float* sin_t, int R, int B, int S, int H, int D,
                            int L, const float* x2, int ldx2, long long bsx2, void* cache2, float* scales2,
                            float* deq2, hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || (D != 64 && D != 128) || L <= 0 || S > L || ldx < H * D || !x || !cache ||
      !scales || !pos || (B > 1 && bsx < (long long)(S - 1) * ldx + H * D) || ((uintptr_t)cache & 15) ||
      ((uintptr_t)scales & 3) || ((uintptr_t)x & 3) || ((uintptr_t)deq & 3) ||
      ((cos_t == nullptr) != (sin_t == nullptr)) || (cos_t && R <= 0) || ((x2 == nullptr) != (cache2 == nullptr)) ||
      ((x2 == nullptr) != (scales2 == nullptr)) || (!x2 && deq2) ||
      (x2 && (ldx2 < H * D || (B > 1 && bsx2 < (long long)(S - 1) * ldx2 + H * D) || ((uintptr_t)cache2 & 15) ||
              ((uintptr_t)scales2 & 3) || ((uintptr_t)x2 & 3) || ((uintptr_t)deq2 & 3))))
    return (int)hipErrorInvalidValue;
  const long long rows = (long long)B * S * H;
  const dim3 grid((unsigned)((rows + 3) / 4), x2 ? 2u : 1u);
  const KvPairQ8 v2{x2, ldx2, bsx2, static_cast<signed char*>(cache2), scales2, deq2};
  if (D == 64)
    hipLaunchKernelGGL(kv_write_q8_kernel<64>, grid, dim3(256), 0, stream, x, ldx, bsx, static_cast<signed char*>(cache),
                       scales, deq, pos, cos_t, sin_t, R, B, S, H, L, v2);
  else
    hipLaunchKernelGGL(kv_write_q8_kernel<128>, grid, dim3(256), 0, stream, x, ldx, bsx,
                       static_cast<signed char*>(cache), scales, deq, pos, cos_t, sin_t, R, B, S, H, L, v2);
  return (int)hipGetLastError();
}

NOS_API int nos_rotary_pos(const void* x, int ldx, long long bsx, void* y, const int* pos, const float* cos_t,
                           const float* sin_t, int R, int B, int S, int H, int D, int bf16, hipStream_t stream) {
  if (B <= 0 || S <= 0 || H <= 0 || D <= 0 || (D % 2) || R <= 0 || ldx < H * D || !cos_t || !sin_t || !pos ||
      (B > 1 && bsx < (long long)(S - 1) * ldx + H * D) || (bf16 != 0 && bf16 != 1))
    return (int)hipErrorInvalidValue;
  const long long n = (long long)B * S * H * (D / 2);
  hipLaunchKernelGGL(rotary_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, ldx, bsx, y, pos,
                     cos_t, sin_t, R, B, S, H, D, bf16);
  return (int)hipGetLastError();
}

// bytes of nos_attn_decode's workspace
NOS_API long long nos_attn_decode_workspace(int B, int H, int Hkv, int Sq, int L, int D) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || Sq <= 0 || L <= 0 || H % Hkv) return -1;
  const int G = H / Hkv, rows = G * (Sq < MAXR / G ? Sq : (MAXR / G > 0 ? MAXR / G : 1));
  const long long NS = (L + KC - 1) / KC;
  return (long long)B * Hkv * NS * rows * (D + 2) * 4;
}

// q [B, Sq, H, D] (heads contiguous per token; token stride ldq, batch stride
// bsq; fp32 / bf16), caches [B, L, Hkv, D] contiguous (fp32 / bf16), pos [B]
// i32: query i at position pos[b] + i sees keys 0 .. min(pos[b] + i, L - 1).
// cos / sin [R, D] fp32 (or null): q rotated at its positions.  out [B, Sq, H,
// D] contiguous (obf: bf16).  Query tokens are processed in launches of at
// most 32 / G (the rows a workgroup holds), each a decode pass + combine.
// kn / vn (nfresh > 0): the step's own K / V rows [B, nfresh, Hkv, D] (token stride
// ldk / ldv, batch stride bsk / bsv; nbf: bf16) -- written into the caches at
// pos[b] + t (K rotated with cos / sin) by the attention itself, which reads them
// from there: the kv_write launch of the step folded in (nfresh == Sq).  sync
// (sync_n >= B x Hkv i32, zero before the first call, left zero by each): the
// combine folded into the decode launch (its last workgroup per (b, kv head)).
// cbf 2: int8 caches with their row scales ks / vs (nos_attn_decode_q8)
static int attn_decode_launch(const void* q, int qbf, int ldq, long long bsq, const void* kc, const void* vc, int cbf,
                              float* ks, float* vs, const int* pos, const float* cos_t, const float* sin_t, int R,
                              void* out, int obf, int B, int H, int Hkv, int Sq, int L, int D, float scale, void* ws,
                              long long ws_bytes, const void* kn, const void* vn, int nbf, int ldk, long long bsk,
                              int ldv, long long bsv, int nfresh, int* sync, long long sync_n, int partials_only,
                              bool ring, int window, int limit, hipStream_t stream) {
  // ring caches (L = C slots): the window and the limit checked before anything else
  if (ring && (L <= 0 || Sq <= 0 || !ring_ok(L, Sq, window, limit, cos_t != nullptr, R)))
    return (int)hipErrorInvalidValue;
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || H / Hkv > MAXR || Sq <= 0 || L <= 0 || (D != 64 && D != 128) ||
      ldq < H * D || (B > 1 && bsq < (long long)(Sq - 1) * ldq + H * D) || !q || !kc || !vc || !pos || !out ||
      !ws || ((cos_t == nullptr) != (sin_t == nullptr)) || (cos_t && R <= 0) || (qbf != 0 && qbf != 1) ||
      (cbf != 0 && cbf != 1 && cbf != 2) || (obf != 0 && obf != 1) || !(scale > 0.f))
    return (int)hipErrorInvalidValue;
  // int8 rows load as 16-byte pieces; fp32 q, rows and output only (an fp32 tenant's storage format)
  if (cbf == 2 && (!ks || !vs || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15) || ((uintptr_t)ks & 3) ||
                   ((uintptr_t)vs & 3) || qbf || obf || (nfresh != 0 && nbf)))
    return (int)hipErrorInvalidValue;
  if (ws_bytes < nos_attn_decode_workspace(B, H, Hkv, Sq, L, D)) return (int)hipErrorInvalidValue;
  if (sync != nullptr && sync_n < (long long)B * Hkv) return (int)hipErrorInvalidValue;
  // partials_only: the splits' partials stay in ws for nos_gemv_partials (one query token)
  if (partials_only && (sync != nullptr || Sq != 1)) return (int)hipErrorInvalidValue;
  Fresh fr;
  if (nfresh != 0) {
    if (nfresh != Sq || !kn || !vn || (nbf != 0 && nbf != 1) || ldk < Hkv * D || ldv < Hkv * D ||
        (B > 1 && (bsk < (long long)(Sq - 1) * ldk + Hkv * D || bsv < (long long)(Sq - 1) * ldv + Hkv * D)))
      return (int)hipErrorInvalidValue;
    fr.k = kn;
    fr.v = vn;
    fr.kc = const_cast<void*>(kc);
    fr.vc = const_cast<void*>(vc);
    fr.bsk = bsk;
    fr.bsv = bsv;
    fr.ldk = ldk;
    fr.ldv = ldv;
    fr.bf = nbf;
    fr.n = nfresh;
  }
  const int G = H / Hkv, chunk = MAXR / G;
  const int NS = (L + KC - 1) / KC;
  for (int q0 = 0; q0 < Sq; q0 += chunk) {
    const int sq = Sq - q0 < chunk ? Sq - q0 : chunk;
    const unsigned grid = (unsigned)(B * Hkv * NS);
    const unsigned rows = (unsigned)(B * Hkv * G * sq);
#define NOS_ATTN_DECODE_R(d, c, r, rg, ...)                                                                        \
  hipLaunchKernelGGL((attn_decode_kernel<d, c, r>), dim3(grid), dim3(256), 0, stream, q, qbf, ldq, bsq, kc, vc, cbf,    \
                     pos, cos_t, sin_t, R, static_cast<float*>(ws), B, H, Hkv, sq, q0, L, NS, scale, fr, sync, out, obf, \
                     Sq, CacheScales<c>{__VA_ARGS__}, rg)
#define NOS_ATTN_DECODE(d, c, ...)                                              \
  do {                                                                          \
    if (ring) {                                                                 \
      NOS_ATTN_DECODE_R(d, c, true, (RingArgs<true>{window, limit}), __VA_ARGS__); \
    } else {                                                                    \
      NOS_ATTN_DECODE_R(d, c, false, RingArgs<false>{}, __VA_ARGS__);           \
    }                                                                           \
  } while (0)
    if (D == 64) {
      if (cbf == 2)
        NOS_ATTN_DECODE(64, 2, ks, vs);
      else if (cbf)
        NOS_ATTN_DECODE(64, 1);
      else
        NOS_ATTN_DECODE(64, 0);
      if (!sync && !partials_only)
        hipLaunchKernelGGL(attn_decode_combine_kernel<64>, dim3(rows), dim3(64), 0, stream,
                           static_cast<const float*>(ws), out, obf, B, H, Hkv, sq, q0, Sq, NS);
    } else {
      if (cbf == 2)
        NOS_ATTN_DECODE(128, 2, ks, vs);
      else if (cbf)
        NOS_ATTN_DECODE(128, 1);
      else
        NOS_ATTN_DECODE(128, 0);
      if (!sync && !partials_only)
        hipLaunchKernelGGL(attn_decode_combine_kernel<128>, dim3(rows), dim3(128), 0, stream,
                           static_cast<const float*>(ws), out, obf, B, H, Hkv, sq, q0, Sq, NS);
    }
  }
#undef NOS_ATTN_DECODE
#undef NOS_ATTN_DECODE_R
  return (int)hipGetLastError();
}

NOS_API int nos_attn_decode(const void* q, int qbf, int ldq, long long bsq, const void* kc, const void* vc, int cbf,
                            const int* pos, const float* cos_t, const float* sin_t, int R, void* out, int obf, int B,
                            int H, int Hkv, int Sq, int L, int D, float scale, void* ws, long long ws_bytes,
                            const void* kn, const void* vn, int nbf, int ldk, long long bsk, int ldv, long long bsv,
                            int nfresh, int* sync, long long sync_n, int partials_only, hipStream_t stream) {
  if (cbf != 0 && cbf != 1) return (int)hipErrorInvalidValue;
  return attn_decode_launch(q, qbf, ldq, bsq, kc, vc, cbf, nullptr, nullptr, pos, cos_t, sin_t, R, out, obf, B, H, Hkv,
                            Sq, L, D, scale, ws, ws_bytes, kn, vn, nbf, ldk, bsk, ldv, bsv, nfresh, sync, sync_n,
                            partials_only, false, 0, 0, stream);
}

// nos_attn_decode over ring caches [B, C, Hkv, D] (kv_ring.h) with a sliding window: query i at position
// p = pos[b] + i attends the positions max(0, p - window + 1) .. p, position j in slot j % C; fresh rows go
// to their slots (rows at positions >= limit dropped); a counter outside [0, limit) gives zero rows.
// C >= min(limit, window + Sq - 1), C <= limit, limit <= R with tables.  Workspace, sync and partials as
// nos_attn_decode with L = C.
NOS_API int nos_attn_decode_ring(const void* q, int qbf, int ldq, long long bsq, const void* kc, const void* vc,
                                 int cbf, const int* pos, const float* cos_t, const float* sin_t, int R, void* out,
                                 int obf, int B, int H, int Hkv, int Sq, int C, int D, float scale, void* ws,
                                 long long ws_bytes, const void* kn, const void* vn, int nbf, int ldk, long long bsk,
                                 int ldv, long long bsv, int nfresh, int* sync, long long sync_n, int partials_only,
                                 int window, int limit, hipStream_t stream) {
  if (cbf != 0 && cbf != 1) return (int)hipErrorInvalidValue;
  return attn_decode_launch(q, qbf, ldq, bsq, kc, vc, cbf, nullptr, nullptr, pos, cos_t, sin_t, R, out, obf, B, H, Hkv,
                            Sq, C, D, scale, ws, ws_bytes, kn, vn, nbf, ldk, bsk, ldv, bsv, nfresh, sync, sync_n,
                            partials_only, true, window, limit, stream);
}

// nos_attn_decode over int8 caches [B, L, Hkv, D] (16-byte aligned) with one fp32 scale per row in
// kscales / vscales [B, L, Hkv]: the attention, in fp32, of the values (float)q x scale the caches hold.
// q, out and the fresh rows kn / vn are fp32; fresh rows are quantized into the caches and the scales
// by the launch (which is why those are not const) and attended as stored.
NOS_API int nos_attn_decode_q8(const float* q, int ldq, long long bsq, void* kc, void* vc, float* kscales,
                               float* vscales, const int* pos, const float* cos_t, const float* sin_t, int R,
                               float* out, int B, int H, int Hkv, int Sq, int L, int D, float scale, void* ws,
                               long long ws_bytes, const float* kn, const float* vn, int ldk, long long bsk, int ldv,
                               long long bsv, int nfresh, int* sync, long long sync_n, int partials_only,
                               hipStream_t stream) {
  return attn_decode_launch(q, 0, ldq, bsq, kc, vc, 2, kscales, vscales, pos, cos_t, sin_t, R, out, 0, B, H, Hkv, Sq, L,
                            D, scale, ws, ws_bytes, kn, vn, 0, ldk, bsk, ldv, bsv, nfresh, sync, sync_n,
                            partials_only, false, 0, 0, stream);
}

// nos_attn_decode_ring over int8 ring caches with their row scales [B, C, Hkv]
NOS_API int nos_attn_decode_ring_q8(const float* q, int ldq, long long bsq, void* kc, void* vc, float* kscales,
                                    float* vscales, const int* pos, const float* cos_t, const float* sin_t, int R,
                                    float* out, int B, int H, int Hkv, int Sq, int C, int D, float scale, void* ws,
                                    long long ws_bytes, const float* kn, const float* vn, int ldk, long long bsk,
                                    int ldv, long long bsv, int nfresh, int* sync, long long sync_n,
                                    int partials_only, int window, int limit, hipStream_t stream) {
  return attn_decode_launch(q, 0, ldq, bsq, kc, vc, 2, kscales, vscales, pos, cos_t, sin_t, R, out, 0, B, H, Hkv, Sq, C,
                            D, scale, ws, ws_bytes, kn, vn, 0, ldk, bsk, ldv, bsv, nfresh, sync, sync_n,
                            partials_only, true, window, limit, stream);
}

NOS_API int nos_pos_update(int* pos, int B, int add, int n, hipStream_t stream) {
  if (!pos || B <= 0 || n < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pos_update_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, pos, B, add, n);
  return (int)hipGetLastError();
}

// pos (or null): pos[row] += pos_n after row's maximum (a decode step's
// position advance in the same launch; rows = the sequences)
NOS_API int nos_argmax(const void* x, int bf16, int rows, int L, int ldx, int* out, int* pos, int pos_n,
                       hipStream_t stream) {
  if (!x || !out || rows <= 0 || L <= 0 || ldx < L || (bf16 != 0 && bf16 != 1) || pos_n < 0)
    return (int)hipErrorInvalidValue;
  if (L >= 4096)
    hipLaunchKernelGGL(argmax_kernel<1024>, dim3((unsigned)rows), dim3(1024), 0, stream, x, bf16, rows, L, ldx, out,
                       pos, pos_n);
  else
    hipLaunchKernelGGL(argmax_kernel<256>, dim3((unsigned)rows), dim3(256), 0, stream, x, bf16, rows, L, ldx, out,
                       pos, pos_n);
  return (int)hipGetLastError();
}

// one token per row drawn under ctl = [temperature fp32 bits, top_k, top_p fp32 bits, seed]
// (4 i32 in device memory; all zero: nos_argmax's result); pos as in nos_argmax, and the
// draw's Philox counter is pos[row] before the advance (0 without pos)
static int sample_lds_limit() {
  static int lds_limit = -1;
  if (lds_limit < 0) {
    int dev = 0, v = 0;
    lds_limit = hipGetDevice(&dev) == hipSuccess &&
                        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess
                    ? v
                    : 0;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<1024>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit > 4096 ? lds_limit - 4096 : 0);
    (void)hipGetLastError();
  }
  return lds_limit;
}

// whether nos_sample keeps a row of L logits in LDS (beside the kernel's 4 KB of static LDS)
NOS_API int nos_sample_row_in_lds(int L) { return (long long)L * 4 + 4096 <= sample_lds_limit(); }

NOS_API int nos_sample(const void* x, int bf16, int rows, int L, int ldx, int* out, int* pos, int pos_n,
                       const int* ctl, hipStream_t stream) {
  if (!x || !out || !ctl || rows <= 0 || L <= 0 || ldx < L || (bf16 != 0 && bf16 != 1) || pos_n < 0)
    return (int)hipErrorInvalidValue;
  const int lds_row = nos_sample_row_in_lds(L);
  const size_t lds = lds_row ? (size_t)L * 4 : 0;
  if (L >= 4096)
    hipLaunchKernelGGL(sample_kernel<1024>, dim3((unsigned)rows), dim3(1024), lds, stream, x, bf16, rows, L, ldx, out,
                       pos, pos_n, ctl, lds_row);
  else
    hipLaunchKernelGGL(sample_kernel<256>, dim3((unsigned)rows), dim3(256), lds, stream, x, bf16, rows, L, ldx, out,
                       pos, pos_n, ctl, lds_row);
  return (int)hipGetLastError();
}

// seen [B, W] i32 bitmaps |= ids [B, S] (row stride ld_ids); reset: the rows cleared first
NOS_API int nos_seen_mark(int* seen, int B, int W, const int* ids, int S, long long ld_ids, int vocab, int reset,
                          hipStream_t stream) {
  if (!seen || !ids || B <= 0 || W <= 0 || S <= 0 || ld_ids < S || vocab <= 0 || (long long)vocab > 32ll * W)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(seen_mark_kernel, dim3((unsigned)B), dim3(256), 0, stream, seen, W, ids, S, ld_ids, vocab, reset);
  return (int)hipGetLastError();
}

// out [rows, L] (row stride ldo) = the logits x [rows, L] (row stride ldx) under the repetition
// penalty ctl[0] (fp32 bits; 0 or 1.0: a copy) on the tokens of seen [rows, W], 32 W >= L
NOS_API int nos_penalize(const void* x, int bf16, int rows, int L, long long ldx, void* out, long long ldo,
                         const int* seen, int W, const int* ctl, hipStream_t stream) {
  if (!x || !out || !seen || !ctl || x == out || rows <= 0 || rows > 65535 || L <= 0 || ldx < L || ldo < L ||
      (bf16 != 0 && bf16 != 1) || 32ll * W < L)
    return (int)hipErrorInvalidValue;
  const size_t al = bf16 ? 8 : 16;
  const int vec = ldx % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<size_t>(x) % al == 0 &&
                  reinterpret_cast<size_t>(out) % al == 0;
  hipLaunchKernelGGL(penalize_kernel, dim3((unsigned)((L + 1023) / 1024), (unsigned)rows), dim3(256), 0, stream, x,
                     bf16, L, ldx, out, ldo, seen, W, ctl, vec);
  return (int)hipGetLastError();
}

// the closing steps of a stopping program over B rows (stop_step_kernel); mode: 1 ids_out =
// done ? pad : next, 2 pos += n unless done, 4 done |= id is a stop id -- the pointers a mode
// needs must be there
NOS_API int nos_stop_step(const int* next, int* ids_out, int* pos, int* done, const int* ctl, int B, int n, int mode,
                          hipStream_t stream) {
  if (!done || B <= 0 || n < 0 || mode <= 0 || mode > 7 || ((mode & 5) && (!next || !ctl)) || ((mode & 1) && !ids_out) ||
      ((mode & 2) && !pos))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(stop_step_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, next, ids_out, pos,
                     done, ctl, B, n, mode);
  return (int)hipGetLastError();
}

// hist [B, L] i32 <- ids [B, >= lead] (row stride ld_ids) and tail [B, T] (row stride ld_tail; or
// null, T = 0) from position pos[b] - back on; n (or null): a count per row (hist_write_kernel)
NOS_API int nos_hist_write(int* hist, int B, int L, const int* pos, int back, const int* ids, int lead,
                           long long ld_ids, const int* tail, int T, long long ld_tail, const int* n,
                           hipStream_t stream) {
  if (!hist || !pos || B <= 0 || L <= 0 || back < 0 || lead < 0 || T < 0 || lead + T <= 0 || (lead > 0 && !ids) ||
      (T > 0 && !tail) || ld_ids < (B > 1 ? lead : 0) || ld_tail < (B > 1 ? T : 0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hist_write_kernel, dim3((unsigned)B), dim3(256), 0, stream, hist, L, pos, back, ids, lead, ld_ids,
                     tail, T, ld_tail, n);
  return (int)hipGetLastError();
}

// a verify step's close over B rows (spec_step_kernel); mode: 1 the advance m -> n_acc, 4 pos += m
// (m: n_acc's without 1), 8 the next input -> out [B, K], 15 the whole step, which also writes the
// accepted tokens into hist.  ids, g, out: contiguous [B, K], 2 <= K <= 8; hist [B, L], L <= 2^28.
NOS_API int nos_spec_step(int* hist, int B, int L, int* pos, const int* ids, const int* g, const int* ctl, int* n_acc,
                          int* out, int K, int mode, hipStream_t stream) {
  if (!pos || B <= 0 || L <= 0 || L > (1 << 28) || K < 2 || K > kSpecMaxK ||
      (mode != 1 && mode != 4 && mode != 8 && mode != 15) || ((mode & 1) && (!ids || !g || !ctl)) ||
      ((mode & 5) && !n_acc) || ((mode & 8) && (!hist || !out)))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(spec_step_kernel, dim3((unsigned)B), dim3(256), 0, stream, hist, L, pos, ids, g, ctl, n_acc, out,
                     K, mode);
  return (int)hipGetLastError();
}

// y [M, N] = act(rms(x) x [M, K] . W [N, K]^T + bias) + res, M <= 8; x, y, res
// share x's dtype (xbf), W and bias W's (wbf); K % 4 == 0, rows 16-byte
// (fp32) / 8-byte (bf16) aligned, M x K x 4 <= 64 KiB (the x rows in LDS).
// rms_eps > 0: each x row RMS-normalised first.  grid: up to 16 workgroups per CU
// walk the N / 8 column groups.
static int gemv_launch(const void* x, int xbf, int ldx, const void* w, int wbf, int ldw, const void* bias,
                       const void* res, int ldr, void* y, int ldy, int M, int N, int K, int epi, float rms_eps,
                       Parts pt, hipStream_t stream, const Lora* lo = nullptr);

// the adapter operand of a GEMV over M rows and N weight rows (Lora), checked before any launch
static bool lora_ok(const Lora& lo, int M, int N) {
  return lo.t && lo.B && lo.sel && lo.R >= 4 && lo.R <= LORA_MAX_R && (lo.R % 4) == 0 && lo.n >= 1 && lo.rps >= 1 &&
         lo.ldb >= lo.R && lo.bsb >= (long long)(N - 1) * lo.ldb + lo.R && M >= 1 && N >= 1 &&
         !((uintptr_t)lo.t & 15) && !((uintptr_t)lo.B & 15);
}

// the decode partials as a GEMV's x (nos_gemv_partials): K = Hkv x G x D columns of M sequences
static bool parts_ok(const float* ws, long long ws_n, int NS, int R, int G, int Hkv, int D, int M, int K) {
  return ws && NS > 0 && G > 0 && Hkv > 0 && (D == 64 || D == 128) && R == G && K == Hkv * G * D && M > 0 && M <= 8 &&
         ws_n >= (long long)M * Hkv * NS * R * (D + 2);
}

NOS_API int nos_gemv(const void* x, int xbf, int ldx, const void* w, int wbf, int ldw, const void* bias,
                     const void* res, int ldr, void* y, int ldy, int M, int N, int K, int epi, float rms_eps,
                     hipStream_t stream) {
  if (!x || !w || !y || M <= 0 || M > 8 || N <= 0 || K <= 0 || (K % 4) || ldx < K || ldw < K || ldy < ((epi & EPI_GLU) ? N / 2 : N) ||
      (long long)M * K * 4 > 65536 || (xbf != 0 && xbf != 1) || (wbf != 0 && wbf != 1) ||
      ((epi & EPI_BIAS) && !bias) || ((epi & EPI_RESID) && (!res || ldr < N)) || (ldx % 4) || (ldw % 4) ||
      ((uintptr_t)x & (xbf ? 7 : 15)) || ((uintptr_t)w & (wbf ? 7 : 15)))
    return (int)hipErrorInvalidValue;
  if ((epi & EPI_GLU) && ((N % 2) || (epi & (EPI_RESID | EPI_GELU | EPI_RELU | EPI_SILU)) || ldy < N / 2))
    return (int)hipErrorInvalidValue;
  return gemv_launch(x, xbf, ldx, w, wbf, ldw, bias, res, ldr, y, ldy, M, N, K, epi, rms_eps, Parts{}, stream);
}

// y [M, N] = act(x W^T + b) + R with x = the decode attention's split partials
// (nos_attn_decode with partials_only: ws [M x Hkv, NS, R = G, D + 2] fp32, one
// query token per sequence), combined in the GEMV's x staging: the combine launch
// folded into the O-projection.  ybf: y / R dtype; K = Hkv x G x D.
NOS_API int nos_gemv_partials(const float* ws, long long ws_n, int NS, int R, int G, int Hkv, int D, int ybf,
                              const void* w, int wbf, int ldw, const void* bias, const void* res, int ldr, void* y,
                              int ldy, int M, int N, int K, int epi, hipStream_t stream) {
  if (!ws || NS <= 0 || G <= 0 || Hkv <= 0 || (D != 64 && D != 128) || R != G || K != Hkv * G * D || !w || !y ||
      M <= 0 || M > 8 || N <= 0 || ws_n < (long long)M * Hkv * NS * R * (D + 2) || (long long)M * K * 4 > 65536 ||
      (ybf != 0 && ybf != 1) || (wbf != 0 && wbf != 1) || ((epi & EPI_BIAS) && !bias) ||
      ((epi & EPI_RESID) && (!res || ldr < N)) || ldy < N || (epi & EPI_GLU) || (ldw % 4) || ldw < K ||
      ((uintptr_t)w & (wbf ? 7 : 15)))
    return (int)hipErrorInvalidValue;
  Parts pt;
  pt.ws = ws;
  pt.NS = NS;
  pt.R = R;
  pt.G = G;
  pt.Hkv = Hkv;
  pt.D = D;
  return gemv_launch(nullptr, ybf, K, w, wbf, ldw, bias, res, ldr, y, ldy, M, N, K, epi, 0.f, pt, stream);
}

static int gemv_launch(const void* x, int xbf, int ldx, const void* w, int wbf, int ldw, const void* bias,
                       const void* res, int ldr, void* y, int ldy, int M, int N, int K, int epi, float rms_eps,
                       Parts pt, hipStream_t stream, const Lora* lo) {
  const int ngrp = (epi & EPI_GLU) ? (N / 2 + 3) / 4 : (N + 7) / 8;
  // every column group its own workgroup up to 16 per CU: a vocabulary head (4000 groups) no
  // longer walks 4 groups per workgroup one memory round trip after another
  const int cap = 16 * nos_effective_cus();
  const unsigned grid = (unsigned)(ngrp < cap ? ngrp : cap);
  const size_t lds = (size_t)M * K * 4;
#define NOS_GEMV_KU(m, b, ku)                                                                                         \
  hipLaunchKernelGGL((gemv_kernel<m, b, ku, false>), dim3(grid), dim3(256), lds, stream, x, xbf, ldx, w, wbf, ldw,    \
                     bias, res, ldr, y, ldy, N, K, epi, rms_eps, pt, LoraArg<false>{})
  // the adapter instantiations: fp32 x and W (adapters are an fp32 tenant's)
#define NOS_GEMV_LORA_KU(m, ku)                                                                                        \
  hipLaunchKernelGGL((gemv_kernel<m, 0, ku, true>), dim3(grid), dim3(256), lds, stream, x, xbf, ldx, w, wbf, ldw, bias, \
                     res, ldr, y, ldy, N, K, epi, rms_eps, pt, LoraArg<true>{*lo})
#define NOS_GEMV(m)                                                                                                   \
  if (lo != nullptr) {                                                                                                \
    if (K > 1024)                                                                                                     \
      NOS_GEMV_LORA_KU(m, 12);                                                                                        \
    else                                                                                                              \
      NOS_GEMV_LORA_KU(m, 4);                                                                                         \
  } else if (K > 1024) {                                                                                                     \
    if (wbf)                                                                                                          \
      NOS_GEMV_KU(m, 1, 12);                                                                                          \
    else                                                                                                              \
      NOS_GEMV_KU(m, 0, 12);                                                                                          \
  } else if (wbf) {                                                                                                   \
    NOS_GEMV_KU(m, 1, 4);                                                                                             \
  } else {                                                                                                            \
    NOS_GEMV_KU(m, 0, 4);                                                                                             \
  }
  switch (M) {
    case 1: NOS_GEMV(1); break;
    case 2: NOS_GEMV(2); break;
    case 3: NOS_GEMV(3); break;
    case 4: NOS_GEMV(4); break;
    case 5: NOS_GEMV(5); break;
    case 6: NOS_GEMV(6); break;
    case 7: NOS_GEMV(7); break;
    default: NOS_GEMV(8); break;
  }
#undef NOS_GEMV
#undef NOS_GEMV_LORA_KU
#undef NOS_GEMV_KU
  return (int)hipGetLastError();
}

// y [M, N] fp32 = act(rms(x) gamma x [M, K] . (q [N, K] int8 * wscale [N])^T + bias) + res, M <= 8: the
// decode step of an int8 weight-only tenant (gemv_q8_kernel).  K % 16 == 0, ldw % 16 == 0, q 16-byte
// aligned, M x K x 4 <= 64 KiB; gamma (or null: ones) only with rms_eps > 0.  grid: up to 3 workgroups
// per CU walk the N / 16 column groups.
static int gemv_q8_launch(const float* x, int ldx, const void* wq, int ldw, const float* wscale, const float* gamma,
                          const float* bias, const float* res, int ldr, float* y, int ldy, int M, int N, int K,
                          int epi, float rms_eps, Parts pt, hipStream_t stream, const Lora* lo = nullptr) {
  if (!wq || !wscale || !y || M <= 0 || M > 8 || N <= 0 || K <= 0 || (K % 16) || ldw < K || (ldw % 16) ||
      ((uintptr_t)wq & 15) || (long long)M * K * 4 > 65536 || ((epi & EPI_BIAS) && !bias) ||
      ((epi & EPI_RESID) && (!res || ldr < N)) || ldy < ((epi & EPI_GLU) ? N / 2 : N) ||
      (gamma && (!(rms_eps > 0.f) || ((uintptr_t)gamma & 15))))
    return (int)hipErrorInvalidValue;
  if ((epi & EPI_GLU) && ((N % 2) || (epi & (EPI_RESID | EPI_GELU | EPI_RELU | EPI_SILU))))
    return (int)hipErrorInvalidValue;
  const int ngrp = (epi & EPI_GLU) ? (N / 2 + 7) / 8 : (N + 15) / 16;
  // a vocabulary head (2000 groups): the workgroups a CU holds at once (3 at M = 1) each walk a few
  // groups, the next one's weights prefetched, and stage x once
  const int cap = 3 * nos_effective_cus();
  const unsigned grid = (unsigned)(ngrp < cap ? ngrp : cap);
  const size_t lds = (size_t)M * K * 4;
#define NOS_GEMV_Q8_KU(m, ku)                                                                                     \
  if (lo != nullptr)                                                                                              \
    hipLaunchKernelGGL((gemv_q8_kernel<m, ku, true>), dim3(grid), dim3(256), lds, stream, x, ldx,                 \
                       static_cast<const signed char*>(wq), ldw, wscale, gamma, bias, res, ldr, y, ldy, N, K, epi, \
                       rms_eps, pt, LoraArg<true>{*lo});                                                          \
  else                                                                                                            \
    hipLaunchKernelGGL((gemv_q8_kernel<m, ku, false>), dim3(grid), dim3(256), lds, stream, x, ldx,                \
                       static_cast<const signed char*>(wq), ldw, wscale, gamma, bias, res, ldr, y, ldy, N, K, epi, \
                       rms_eps, pt, LoraArg<false>{})
  // K <= 1024: the whole row in one batch of Q8_R loads per lane; longer rows (a down projection's
  // 2816) in batches of 3 x Q8_R
#define NOS_GEMV_Q8(m)      \
  if (K > 1024) {           \
    NOS_GEMV_Q8_KU(m, 3);   \
  } else {                  \
    NOS_GEMV_Q8_KU(m, 1);   \
  }
  switch (M) {
    case 1: NOS_GEMV_Q8(1); break;
    case 2: NOS_GEMV_Q8(2); break;
    case 3: NOS_GEMV_Q8(3); break;
    case 4: NOS_GEMV_Q8(4); break;
    case 5: NOS_GEMV_Q8(5); break;
    case 6: NOS_GEMV_Q8(6); break;
    case 7: NOS_GEMV_Q8(7); break;
    default: NOS_GEMV_Q8(8); break;
  }
#undef NOS_GEMV_Q8
#undef NOS_GEMV_Q8_KU
  return (int)hipGetLastError();
}

NOS_API int nos_gemv_q8(const float* x, int ldx, const void* wq, int ldw, const float* wscale, const float* gamma,
                        const float* bias, const float* res, int ldr, float* y, int ldy, int M, int N, int K, int epi,
                        float rms_eps, hipStream_t stream) {
  if (!x || ldx < K || (ldx % 4) || ((uintptr_t)x & 15)) return (int)hipErrorInvalidValue;
  return gemv_q8_launch(x, ldx, wq, ldw, wscale, gamma, bias, res, ldr, y, ldy, M, N, K, epi, rms_eps, Parts{},
                        stream);
}

// nos_gemv_q8 with x = the decode attention's split partials (as nos_gemv_partials): the combine
// launch folded into an int8 O-projection
NOS_API int nos_gemv_q8_partials(const float* ws, long long ws_n, int NS, int R, int G, int Hkv, int D, const void* wq,
                                 int ldw, const float* wscale, const float* bias, const float* res, int ldr, float* y,
                                 int ldy, int M, int N, int K, int epi, hipStream_t stream) {
  if (!ws || NS <= 0 || G <= 0 || Hkv <= 0 || (D != 64 && D != 128) || R != G || K != Hkv * G * D || M <= 0 ||
      M > 8 || ws_n < (long long)M * Hkv * NS * R * (D + 2) || (epi & EPI_GLU))
    return (int)hipErrorInvalidValue;
  Parts pt;
  pt.ws = ws;
  pt.NS = NS;
  pt.R = R;
  pt.G = G;
  pt.Hkv = Hkv;
  pt.D = D;
  return gemv_q8_launch(nullptr, K, wq, ldw, wscale, nullptr, bias, res, ldr, y, ldy, M, N, K, epi, 0.f, pt, stream);
}

// The LoRA shrink in front of an adapted GEMV (lora_shrink_kernel): t [M, R] fp32 (contiguous) from x
// [M, K] fp32 -- or, with ws, from the decode partials (as nos_gemv_partials; x is then unused, rps 1
// and no RMSNorm) -- and A [n, R, K] fp32 (adapter stride bsa, row stride lda, 16-byte rows).  M <= 8,
// 4 <= R <= 64 with R % 4 == 0, K % 4 == 0, M x K x 4 <= 64 KiB (the GEMV's own bound); gamma (or
// null) only with rms_eps > 0.  sel holds at least ceil(M / rps) ids.
NOS_API int nos_lora_shrink(const float* x, int ldx, const float* ws, long long ws_n, int NS, int G, int Hkv, int D,
                            const float* A, long long bsa, int lda, const int* sel, int n, int rps, const float* gamma,
                            float rms_eps, float* t, int M, int R, int K, hipStream_t stream) {
  if (!A || !sel || !t || M <= 0 || M > 8 || R < 4 || R > LORA_MAX_R || (R % 4) || K <= 0 || (K % 4) || n < 1 ||
      rps < 1 || lda < K || (lda % 4) || bsa < (long long)(R - 1) * lda + K || (bsa % 4) || ((uintptr_t)A & 15) ||
      ((uintptr_t)t & 15) || (long long)M * K * 4 > 65536 || (gamma && (!(rms_eps > 0.f) || ((uintptr_t)gamma & 15))))
    return (int)hipErrorInvalidValue;
  Parts pt;
  if (ws != nullptr) {
    if (!parts_ok(ws, ws_n, NS, G, G, Hkv, D, M, K) || rps != 1 || rms_eps > 0.f) return (int)hipErrorInvalidValue;
    pt.ws = ws;
    pt.NS = NS;
    pt.R = G;
    pt.G = G;
    pt.Hkv = Hkv;
    pt.D = D;
    ldx = K;
  } else if (!x || ldx < K || (ldx % 4) || ((uintptr_t)x & 15)) {
    return (int)hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(lora_shrink_kernel, dim3((unsigned)(M * (R / 4))), dim3(256), 0, stream, x, ldx, A, bsa, lda,
                     sel, n, rps, gamma, rms_eps, t, M, R, K, pt);
  return (int)hipGetLastError();
}

// nos_gemv / nos_gemv_partials (ws != null: x is unused) of fp32 x and W with the adapter epilogue
// (Lora): y gets + sum_j B[sel[m / rps] - 1][n][j] t[m][j] before bias, activation, GLU or residual.
NOS_API int nos_gemv_lora(const float* x, int ldx, const float* ws, long long ws_n, int NS, int G, int Hkv, int D,
                          const float* w, int ldw, const float* bias, const float* res, int ldr, float* y, int ldy,
                          int M, int N, int K, int epi, float rms_eps, const float* t, const float* B, long long bsb,
                          int ldb, const int* sel, int R, int n, int rps, hipStream_t stream) {
  Lora lo;
  lo.t = t;
  lo.B = B;
  lo.sel = sel;
  lo.bsb = bsb;
  lo.ldb = ldb;
  lo.R = R;
  lo.n = n;
  lo.rps = rps;
  if (!w || !y || M <= 0 || M > 8 || N <= 0 || K <= 0 || (K % 4) || ldw < K || (ldw % 4) || ((uintptr_t)w & 15) ||
      ldy < ((epi & EPI_GLU) ? N / 2 : N) || (long long)M * K * 4 > 65536 || ((epi & EPI_BIAS) && !bias) ||
      ((epi & EPI_RESID) && (!res || ldr < N)) || !lora_ok(lo, M, N))
    return (int)hipErrorInvalidValue;
  if ((epi & EPI_GLU) && ((N % 2) || (epi & (EPI_RESID | EPI_GELU | EPI_RELU | EPI_SILU)))) return (int)hipErrorInvalidValue;
  Parts pt;
  if (ws != nullptr) {
    if (!parts_ok(ws, ws_n, NS, G, G, Hkv, D, M, K) || (epi & EPI_GLU) || rps != 1 || rms_eps > 0.f)
      return (int)hipErrorInvalidValue;
    pt.ws = ws;
    pt.NS = NS;
    pt.R = G;
    pt.G = G;
    pt.Hkv = Hkv;
    pt.D = D;
    return gemv_launch(nullptr, 0, K, w, 0, ldw, bias, res, ldr, y, ldy, M, N, K, epi, 0.f, pt, stream, &lo);
  }
  if (!x || ldx < K || (ldx % 4) || ((uintptr_t)x & 15)) return (int)hipErrorInvalidValue;
  return gemv_launch(x, 0, ldx, w, 0, ldw, bias, res, ldr, y, ldy, M, N, K, epi, rms_eps, pt, stream, &lo);
}

// nos_gemv_q8 / nos_gemv_q8_partials (ws != null: x is unused) with the adapter epilogue, as nos_gemv_lora
NOS_API int nos_gemv_q8_lora(const float* x, int ldx, const float* ws, long long ws_n, int NS, int G, int Hkv, int D,
                             const void* wq, int ldw, const float* wscale, const float* gamma, const float* bias,
                             const float* res, int ldr, float* y, int ldy, int M, int N, int K, int epi, float rms_eps,
                             const float* t, const float* B, long long bsb, int ldb, const int* sel, int R, int n,
                             int rps, hipStream_t stream) {
  Lora lo;
  lo.t = t;
  lo.B = B;
  lo.sel = sel;
  lo.bsb = bsb;
  lo.ldb = ldb;
  lo.R = R;
  lo.n = n;
  lo.rps = rps;
  if (M <= 0 || M > 8 || N <= 0 || !lora_ok(lo, M, N)) return (int)hipErrorInvalidValue;
  Parts pt;
  if (ws != nullptr) {
    if (!parts_ok(ws, ws_n, NS, G, G, Hkv, D, M, K) || (epi & EPI_GLU) || rps != 1 || rms_eps > 0.f || gamma)
      return (int)hipErrorInvalidValue;
    pt.ws = ws;
    pt.NS = NS;
    pt.R = G;
    pt.G = G;
    pt.Hkv = Hkv;
    pt.D = D;
    return gemv_q8_launch(nullptr, K, wq, ldw, wscale, nullptr, bias, res, ldr, y, ldy, M, N, K, epi, 0.f, pt, stream,
                          &lo);
  }
  if (!x || ldx < K || (ldx % 4) || ((uintptr_t)x & 15)) return (int)hipErrorInvalidValue;
  return gemv_q8_launch(x, ldx, wq, ldw, wscale, gamma, bias, res, ldr, y, ldy, M, N, K, epi, rms_eps, pt, stream, &lo);
}

// out [N, K] fp32 (row stride ldo) = (float)q [N, K] int8 * wscale [N], bit-exact: the weight of an
// int8 linear at more than 8 rows, for the h3 product.  K, ldw % 4 == 0, ldo % 4 == 0, out 16-byte aligned.
NOS_API int nos_dequant_q8(const void* wq, int ldw, const float* wscale, float* out, int ldo, int N, int K,
                           hipStream_t stream) {
  if (!wq || !wscale || !out || N <= 0 || K <= 0 || (K % 4) || ldw < K || (ldw % 4) || ldo < K || (ldo % 4) ||
      ((uintptr_t)wq & 3) || ((uintptr_t)out & 15))
    return (int)hipErrorInvalidValue;
  const long long total = (long long)N * (K / 4);
  const long long cap = 32LL * nos_effective_cus();
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(dequant_q8_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, stream,
                     static_cast<const signed char*>(wq), ldw, wscale, out, ldo, N, K);
  return (int)hipGetLastError();
}

// y [M, N] fp32 = act(rms(x) gamma x [M, K] . dequant(codes [N, K / 2], scales [N, K / 32])^T + bias) + res,
// M <= 8: the decode step of an MXFP4 weight-only tenant (gemv_mx4_kernel).  K % 32 == 0, ldw (bytes
// per row of codes) % 16 == 0, codes 16-byte aligned, ldsc >= K / 32, M x K x 4 <= 64 KiB; gamma (or
// null: ones) only with rms_eps > 0.  Every scale byte must lie in [2, 252] (the registration checks
// it).  grid: as the int8 GEMV's.
#ifndef NOS_MX4_NARROW_K
#define NOS_MX4_NARROW_K 1024   // rows up to this long take the 8-byte-load form (docs/kernels.md)
#endif
static int gemv_mx4_launch(const float* x, int ldx, const void* wq, int ldw, const void* wscale, int ldsc,
                           const float* gamma, const float* bias, const float* res, int ldr, float* y, int ldy, int M,
                           int N, int K, int epi, float rms_eps, Parts pt, hipStream_t stream) {
  if (!wq || !wscale || !y || M <= 0 || M > 8 || N <= 0 || K <= 0 || (K % 32) || ldw < K / 2 || (ldw % 16) ||
      ((uintptr_t)wq & 15) || ldsc < K / 32 || (long long)M * K * 4 > 65536 || ((epi & EPI_BIAS) && !bias) ||
      ((epi & EPI_RESID) && (!res || ldr < N)) || ldy < ((epi & EPI_GLU) ? N / 2 : N) ||
      (gamma && (!(rms_eps > 0.f) || ((uintptr_t)gamma & 15))))
    return (int)hipErrorInvalidValue;
  if ((epi & EPI_GLU) && ((N % 2) || (epi & (EPI_RESID | EPI_GELU | EPI_RELU | EPI_SILU))))
    return (int)hipErrorInvalidValue;
  const int ngrp = (epi & EPI_GLU) ? (N / 2 + 7) / 8 : (N + 15) / 16;
  const int cap = 3 * nos_effective_cus();
  const unsigned grid = (unsigned)(ngrp < cap ? ngrp : cap);
  const size_t lds = (size_t)M * K * 4;
#define NOS_GEMV_MX4_F(m, ku, lb)                                                                                  \
  hipLaunchKernelGGL((gemv_mx4_kernel<m, ku, lb>), dim3(grid), dim3(256), lds, stream, x, ldx,                     \
                     static_cast<const unsigned char*>(wq), ldw, static_cast<const unsigned char*>(wscale), ldsc, \
                     gamma, bias, res, ldr, y, ldy, N, K, epi, rms_eps, pt)
  // K <= 1024: 8-byte loads, the whole row in one batch with every lane at work (148 against 194
  // VGPRs at M = 1, and measured alone against the 16-byte form: 3.60 / 3.86 us at 1024 x 1024,
  // 8.95 / 12.80 us at the 32000 x 1024 head); K <= 2048: one block per lane; longer rows (a down
  // projection's 2816) in batches of 2 x MX4_R loads
#define NOS_GEMV_MX4(m)                \
  if (K <= NOS_MX4_NARROW_K) {         \
    NOS_GEMV_MX4_F(m, 1, 8);           \
  } else if (K <= 2048) {              \
    NOS_GEMV_MX4_F(m, 1, 16);          \
  } else {                             \
    NOS_GEMV_MX4_F(m, 2, 16);          \
  }
  switch (M) {
    case 1: NOS_GEMV_MX4(1); break;
    case 2: NOS_GEMV_MX4(2); break;
    case 3: NOS_GEMV_MX4(3); break;
    case 4: NOS_GEMV_MX4(4); break;
    case 5: NOS_GEMV_MX4(5); break;
    case 6: NOS_GEMV_MX4(6); break;
    case 7: NOS_GEMV_MX4(7); break;
    default: NOS_GEMV_MX4(8); break;
  }
#undef NOS_GEMV_MX4
#undef NOS_GEMV_MX4_F
  return (int)hipGetLastError();
}

NOS_API int nos_gemv_mx4(const float* x, int ldx, const void* wq, int ldw, const void* wscale, int ldsc,
                         const float* gamma, const float* bias, const float* res, int ldr, float* y, int ldy, int M,
                         int N, int K, int epi, float rms_eps, hipStream_t stream) {
  if (!x || ldx < K || (ldx % 4) || ((uintptr_t)x & 15)) return (int)hipErrorInvalidValue;
  return gemv_mx4_launch(x, ldx, wq, ldw, wscale, ldsc, gamma, bias, res, ldr, y, ldy, M, N, K, epi, rms_eps, Parts{},
                         stream);
}

// nos_gemv_mx4 with x = the decode attention's split partials (as nos_gemv_partials): the combine
// launch folded into an MXFP4 O-projection
NOS_API int nos_gemv_mx4_partials(const float* ws, long long ws_n, int NS, int R, int G, int Hkv, int D,
                                  const void* wq, int ldw, const void* wscale, int ldsc, const float* bias,
                                  const float* res, int ldr, float* y, int ldy, int M, int N, int K, int epi,
                                  hipStream_t stream) {
  if (!parts_ok(ws, ws_n, NS, R, G, Hkv, D, M, K) || (epi & EPI_GLU)) return (int)hipErrorInvalidValue;
  Parts pt;
  pt.ws = ws;
  pt.NS = NS;
  pt.R = R;
  pt.G = G;
  pt.Hkv = Hkv;
  pt.D = D;
  return gemv_mx4_launch(nullptr, K, wq, ldw, wscale, ldsc, nullptr, bias, res, ldr, y, ldy, M, N, K, epi, 0.f, pt,
                         stream);
}

// out [N, K] fp32 (row stride ldo) = the MXFP4 weight dequantized, bit-exact: the weight of an MXFP4
// linear at more than 8 rows, for the h3 product.  K % 32 == 0, ldw % 4 == 0, ldo % 4 == 0, codes
// 4-byte and out 16-byte aligned.
NOS_API int nos_dequant_mx4(const void* wq, int ldw, const void* wscale, int ldsc, float* out, int ldo, int N, int K,
                            hipStream_t stream) {
  if (!wq || !wscale || !out || N <= 0 || K <= 0 || (K % 32) || ldw < K / 2 || (ldw % 4) || ldsc < K / 32 || ldo < K ||
      (ldo % 4) || ((uintptr_t)wq & 3) || ((uintptr_t)out & 15))
    return (int)hipErrorInvalidValue;
  const long long total = (long long)N * (K / 8);
  const long long cap = 32LL * nos_effective_cus();
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(dequant_mx4_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, stream,
                     static_cast<const unsigned char*>(wq), ldw, static_cast<const unsigned char*>(wscale), ldsc, out,
                     ldo, N, K);
  return (int)hipGetLastError();
}

// The mixture-of-experts block of a decode step (moe_route_kernel / moe_glu_kernel / moe_down_kernel):
// M <= 8 rows of x [M, H] fp32, E <= 64 experts, 1 <= k <= min(E, 8), H % 4 == 0 and I % 4 == 0, every
// base 16-byte aligned and every row stride a multiple of 4 floats; gamma (or null) only with
// rms_eps > 0.  idx [M, k] i32 and w [M, k] fp32 are contiguous, act [M, k, I] fp32 too.
static bool moe_dims_ok(int M, int E, int H, int I, int k) {
  return M >= 1 && M <= 8 && E >= 1 && E <= MOE_MAX_E && k >= 1 && k <= MOE_MAX_K && k <= E && H >= 4 && (H % 4) == 0 &&
         I >= 4 && (I % 4) == 0 && (long long)H * 4 <= 65536;
}

static bool moe_x_ok(const float* x, int ldx, const float* gamma, float rms_eps, int H) {
  return x && ldx >= H && (ldx % 4) == 0 && !((uintptr_t)x & 15) &&
         (!gamma || (rms_eps > 0.f && !((uintptr_t)gamma & 15)));
}

NOS_API int nos_moe_route(const float* x, int ldx, const float* Wr, int ldwr, const float* gamma, float rms_eps,
                          int* idx, float* w, int M, int E, int H, int k, hipStream_t stream) {
  if (!moe_dims_ok(M, E, H, 4, k) || !moe_x_ok(x, ldx, gamma, rms_eps, H) || !Wr || ldwr < H || (ldwr % 4) ||
      ((uintptr_t)Wr & 15) || !idx || !w || ((uintptr_t)idx & 3) || ((uintptr_t)w & 3))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(moe_route_kernel, dim3((unsigned)M), dim3(256), (size_t)H * 4, stream, x, ldx, Wr, ldwr, gamma,
                     rms_eps, idx, w, E, H, k);
  return (int)hipGetLastError();
}

NOS_API int nos_moe_glu(const float* x, int ldx, const int* idx, const float* W13, long long bs13, int ld13,
                        const float* gamma, float rms_eps, float* act, int M, int E, int H, int I, int k,
                        hipStream_t stream) {
  if (!moe_dims_ok(M, E, H, I, k) || !moe_x_ok(x, ldx, gamma, rms_eps, H) || !idx || ((uintptr_t)idx & 3) || !W13 ||
      ld13 < H || (ld13 % 4) || bs13 < (long long)(2 * I - 1) * ld13 + H || (bs13 % 4) || ((uintptr_t)W13 & 15) ||
      !act || ((uintptr_t)act & 15))
    return (int)hipErrorInvalidValue;
  const int ngrp = (I + 3) / 4, pairs = M * k;
  int gx = 16 * nos_effective_cus() / pairs;   // up to 16 workgroups per CU over all pairs, as the GEMV
  gx = gx < 1 ? 1 : (gx > ngrp ? ngrp : gx);
  hipLaunchKernelGGL(moe_glu_kernel, dim3((unsigned)gx, (unsigned)pairs), dim3(256), (size_t)H * 4, stream, x, ldx,
                     idx, W13, bs13, ld13, gamma, rms_eps, act, E, H, I, k);
  return (int)hipGetLastError();
}

NOS_API int nos_moe_down(const float* act, const int* idx, const float* w, const float* W2, long long bs2, int ld2,
                         const float* res, int ldr, float* y, int ldy, int M, int E, int H, int I, int k,
                         hipStream_t stream) {
  if (!moe_dims_ok(M, E, H, I, k) || (long long)k * I * 4 > 65536 || !act || ((uintptr_t)act & 15) || !idx ||
      ((uintptr_t)idx & 3) || !w || ((uintptr_t)w & 3) || !W2 || ld2 < I || (ld2 % 4) ||
      bs2 < (long long)(H - 1) * ld2 + I || (bs2 % 4) || ((uintptr_t)W2 & 15) || !y || ((uintptr_t)y & 3) || ldy < H ||
      (res && (ldr < H || ((uintptr_t)res & 3))))
    return (int)hipErrorInvalidValue;
  const int ngrp = (H + 3) / 4;
  int gx = 16 * nos_effective_cus() / M;
  gx = gx < 1 ? 1 : (gx > ngrp ? ngrp : gx);
  hipLaunchKernelGGL(moe_down_kernel, dim3((unsigned)gx, (unsigned)M), dim3(256), (size_t)k * I * 4, stream, act, idx,
                     w, W2, bs2, ld2, res, ldr, y, ldy, E, H, I, k);
  return (int)hipGetLastError();
}

// nos_moe_glu / nos_moe_down over quantized experts (moe_glu_quant_kernel / moe_down_quant_kernel; the
// route launch is nos_moe_route).  The fp32 entry points' contract, and: H and I multiples of KM (16 for
// int8, 32 for MXFP4); codes 16-byte aligned with row and expert strides (bytes) that are multiples of 16;
// int8 scales fp32 [E, rows] with an expert stride bss (floats); MXFP4 scale bytes [E, rows, K / 32] with
// strides bss >= rows x lds and lds >= K / 32 (bytes), every byte in [2, 252] (the registration checks it).
static bool moe_quant_ok(int M, int E, int H, int I, int k, int KM, const void* Wq, long long bsw, int ldw,
                         int rows, int kbytes, const void* S) {
  return moe_dims_ok(M, E, H, I, k) && (H % KM) == 0 && (I % KM) == 0 && Wq && !((uintptr_t)Wq & 15) &&
         ldw >= kbytes && (ldw % 16) == 0 && bsw >= (long long)(rows - 1) * ldw + kbytes && (bsw % 16) == 0 && S;
}

static int moe_glu_quant_grid(int I, int pairs) {
  const int ngrp = (I + 7) / 8;
  const int gx = 16 * nos_effective_cus() / pairs;   // up to 16 workgroups per CU over all pairs, as nos_moe_glu
  return gx < 1 ? 1 : (gx > ngrp ? ngrp : gx);
}

template <class F>
static int moe_glu_quant_launch(const float* x, int ldx, const int* idx, const void* Wq, long long bsw, int ldw,
                                const void* S, long long bss, int lds, const float* gamma, float rms_eps, float* act,
                                int M, int E, int H, int I, int k, hipStream_t stream) {
  hipLaunchKernelGGL((moe_glu_quant_kernel<F>), dim3((unsigned)moe_glu_quant_grid(I, M * k), (unsigned)(M * k)),
                     dim3(256), (size_t)H * 4, stream, x, ldx, idx, static_cast<const unsigned char*>(Wq), bsw, ldw, S,
                     bss, lds, gamma, rms_eps, act, E, H, I, k);
  return (int)hipGetLastError();
}

// R = 2 columns per wave where the grid still covers the CUs, else a column per wave (a single row of
// H = 1024: 256 workgroups, as nos_moe_down)
template <class F>
static int moe_down_quant_launch(const float* act, const int* idx, const float* w, const void* Wq, long long bsw,
                                 int ldw, const void* S, long long bss, int lds, const float* res, int ldr, float* y,
                                 int ldy, int M, int E, int H, int I, int k, hipStream_t stream) {
  const int cus = nos_effective_cus();
  const bool wide = (long long)M * ((H + 7) / 8) >= cus;
  const int ngrp = wide ? (H + 7) / 8 : (H + 3) / 4;
  int gx = 16 * cus / M;
  gx = gx < 1 ? 1 : (gx > ngrp ? ngrp : gx);
#define NOS_MOE_DOWN_Q(r)                                                                                          \
  hipLaunchKernelGGL((moe_down_quant_kernel<F, r>), dim3((unsigned)gx, (unsigned)M), dim3(256), (size_t)k * I * 4, \
                     stream, act, idx, w, static_cast<const unsigned char*>(Wq), bsw, ldw, S, bss, lds, res, ldr, \
                     y, ldy, E, H, I, k)
  if (wide) {
    NOS_MOE_DOWN_Q(2);
  } else {
    NOS_MOE_DOWN_Q(1);
  }
#undef NOS_MOE_DOWN_Q
  return (int)hipGetLastError();
}

static bool moe_down_args_ok(const float* act, const int* idx, const float* w, const float* res, int ldr,
                             const float* y, int ldy, int H, int I, int k) {
  return (long long)k * I * 4 <= 65536 && act && !((uintptr_t)act & 15) && idx && !((uintptr_t)idx & 3) && w &&
         !((uintptr_t)w & 3) && y && !((uintptr_t)y & 3) && ldy >= H && (!res || (ldr >= H && !((uintptr_t)res & 3)));
}

NOS_API int nos_moe_glu_q8(const float* x, int ldx, const int* idx, const void* W13q, long long bs13, int ld13,
                           const float* s13, long long bss13, const float* gamma, float rms_eps, float* act, int M,
                           int E, int H, int I, int k, hipStream_t stream) {
  if (!moe_quant_ok(M, E, H, I, k, 16, W13q, bs13, ld13, 2 * I, H, s13) || !moe_x_ok(x, ldx, gamma, rms_eps, H) ||
      !idx || ((uintptr_t)idx & 3) || bss13 < 2 * I || ((uintptr_t)s13 & 3) || !act || ((uintptr_t)act & 15))
    return (int)hipErrorInvalidValue;
  return moe_glu_quant_launch<MoeQ8>(x, ldx, idx, W13q, bs13, ld13, s13, bss13, 0, gamma, rms_eps, act, M, E, H, I, k,
                                     stream);
}

NOS_API int nos_moe_down_q8(const float* act, const int* idx, const float* w, const void* W2q, long long bs2, int ld2,
                            const float* s2, long long bss2, const float* res, int ldr, float* y, int ldy, int M,
                            int E, int H, int I, int k, hipStream_t stream) {
  if (!moe_quant_ok(M, E, H, I, k, 16, W2q, bs2, ld2, H, I, s2) || !moe_down_args_ok(act, idx, w, res, ldr, y, ldy, H, I, k) ||
      bss2 < H || ((uintptr_t)s2 & 3))
    return (int)hipErrorInvalidValue;
  return moe_down_quant_launch<MoeQ8>(act, idx, w, W2q, bs2, ld2, s2, bss2, 0, res, ldr, y, ldy, M, E, H, I, k,
                                      stream);
}

// rows up to NOS_MX4_NARROW_K long take the 8-byte-load form, as the MXFP4 GEMV (docs/kernels.md)
NOS_API int nos_moe_glu_mx4(const float* x, int ldx, const int* idx, const void* W13c, long long bs13, int ld13,
                            const void* e13, long long bse13, int lde13, const float* gamma, float rms_eps,
                            float* act, int M, int E, int H, int I, int k, hipStream_t stream) {
  if (!moe_quant_ok(M, E, H, I, k, 32, W13c, bs13, ld13, 2 * I, H / 2, e13) ||
      !moe_x_ok(x, ldx, gamma, rms_eps, H) || !idx || ((uintptr_t)idx & 3) || lde13 < H / 32 ||
      bse13 < (long long)(2 * I - 1) * lde13 + H / 32 || !act || ((uintptr_t)act & 15))
    return (int)hipErrorInvalidValue;
  if (H <= NOS_MX4_NARROW_K)
    return moe_glu_quant_launch<MoeMx4<8>>(x, ldx, idx, W13c, bs13, ld13, e13, bse13, lde13, gamma, rms_eps, act, M, E,
                                           H, I, k, stream);
  return moe_glu_quant_launch<MoeMx4<16>>(x, ldx, idx, W13c, bs13, ld13, e13, bse13, lde13, gamma, rms_eps, act, M, E,
                                          H, I, k, stream);
}

NOS_API int nos_moe_down_mx4(const float* act, const int* idx, const float* w, const void* W2c, long long bs2, int ld2,
                             const void* e2, long long bse2, int lde2, const float* res, int ldr, float* y, int ldy,
                             int M, int E, int H, int I, int k, hipStream_t stream) {
  if (!moe_quant_ok(M, E, H, I, k, 32, W2c, bs2, ld2, H, I / 2, e2) ||
      !moe_down_args_ok(act, idx, w, res, ldr, y, ldy, H, I, k) || lde2 < I / 32 ||
      bse2 < (long long)(H - 1) * lde2 + I / 32)
    return (int)hipErrorInvalidValue;
  if (I <= NOS_MX4_NARROW_K)
    return moe_down_quant_launch<MoeMx4<8>>(act, idx, w, W2c, bs2, ld2, e2, bse2, lde2, res, ldr, y, ldy, M, E, H, I,
                                            k, stream);
  return moe_down_quant_launch<MoeMx4<16>>(act, idx, w, W2c, bs2, ld2, e2, bse2, lde2, res, ldr, y, ldy, M, E, H, I, k,
                                           stream);
}
