// Backward of the general h3 attention (attention_h3g.hip) for training
// tenants: dQ, dK, dV of O = softmax(scale Q K^T [+ causal mask]) V from the
// forward's saved log-sum-exp, on the fp16x3 ("h3") matrix pipes.
//
//   P = exp(scale Q K^T - lse),  dP = dO V^T,  delta_i = rowsum(dO_i . O_i),
//   dS = scale P (dP - delta),   dV = P^T dO,  dK = dS^T Q,  dQ = dS K
//
// Two main kernels, no atomics and no workgroup ever waiting for another, so
// the gradients are the same bits from run to run and nothing is zeroed first:
//
//  * attn_h3g_bwd_dkdv_kernel: one workgroup = 4 waves x 32 keys of one
//    (batch, KV head).  It sweeps the g = H / Hkv query heads of that KV head
//    and their 32-row query tiles (causal: only tiles that see the block) and
//    keeps dK^T and dV^T of its keys in accumulator registers: the
//    grouped-query sum happens there.  When the grid leaves CUs idle the sweep
//    is cut into ranges whose partial sums a merge kernel adds in a fixed order.
//  * attn_h3g_bwd_dq_kernel: one workgroup = 4 waves x 32 query rows of one
//    (batch, head); it sweeps the 32-key tiles and keeps dQ^T in registers.
//
// Both recompute S and dP per tile pair (7 MFMA products instead of 5).
//
// Scales (split_f16.h: an operand is two fp16 pieces on a power-of-two scale
// that is factored out of the accumulator, so it must be constant along the
// reduction):
//  * S reduces over D: Q carries the forward's per-row scale with the softmax
//    scale folded in and K the forward's per-head scale -- the same pieces in
//    the same MFMA order as the forward, so the recomputed scores are the
//    scores the log-sum-exp was taken of;
//  * dP reduces over D, dV^T / dK^T over query rows and the heads of a group:
//    dO, and Q as the operand of dK^T, carry ONE scale per (batch, KV head),
//    measured by the pre-pass like K / V;
//  * P lies in [0, 1]: fixed scale 2^13;
//  * dS carries a proven bound, not a measured one: |dP_ij| <= D max|dO| max|V|,
//    delta_i is a convex combination of dP_ij, so
//    |dS_ij| <= 2 scale D max|dO| max|V| (per batch and KV head).
//
// Pre-pass: the forward's kv_absmax / kv_scale / split_kv (attn_kv_planes.h)
// for K / V, kv_absmax again for Q / dO, then the row planes of Q / dO with
// delta and the per-row constants, and TRANSPOSED planes of K, Q and dO
// ([tile][piece][D][32 rows]): the products that reduce over rows read their
// A operand from those with plain 8-byte LDS reads.  Tiles are staged global
// -> registers -> LDS (padded rows), one tile prefetched in registers while
// the current one is multiplied.
#include <limits.h>
#include <math.h>

#include "attn_kv_planes.h"
#include "common.h"
#include "split_f16.h"

namespace {

constexpr int BW = 4;             // waves per workgroup
constexpr int BLK = 32 * BW;      // keys (dkdv) / query rows (dq) per workgroup
constexpr int TP = 40;            // fp16 per row of a transposed tile image in LDS (32 + pad)
constexpr int MAX_QSPLIT = 8;     // ranges of the dkdv sweep
constexpr int GRP = 8;            // floats per (batch, KV head) in the constants block
constexpr float P_EXP = 13.f;     // P is carried as P 2^13

// grp[(b * Hkv + hk) * GRP + ..]
enum { G_QSC = 0, G_DOSC = 1, G_A1 = 2, G_A2 = 3, G_DVF = 4, G_DKF = 5, G_DQF = 6, G_KINV = 7 };

__device__ __forceinline__ int ub_exp(float v) {  // v < 2^e (v > 0)
  int e;
  frexpf(v, &e);
  return e;
}

// ---------------------------------------------------------------- constants
// one thread per (batch, KV head): the group-wide Q / dO scales, the dS bound
// and the factors that take the accumulators back to true units
__global__ __launch_bounds__(256) void bwd_scale_kernel(const float* __restrict__ kvabs, const float* __restrict__ qabs,
                                                        float* __restrict__ grp, int n, int Hkv, int g, int nck,
                                                        int ncq, float scale, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / Hkv, hk = i - b * Hkv;
  float mk = 0.f, mv = 0.f, mq = 0.f, mdo = 0.f;
  for (int c = 0; c < nck; ++c) {
    mk = fmaxf(mk, kvabs[((long long)i * nck + c) * 2]);
    mv = fmaxf(mv, kvabs[((long long)i * nck + c) * 2 + 1]);
  }
  for (int hg = 0; hg < g; ++hg) {
    const long long bh = (long long)b * Hkv * g + hk * g + hg;
    for (int c = 0; c < ncq; ++c) {
      mq = fmaxf(mq, qabs[(bh * ncq + c) * 2]);
      mdo = fmaxf(mdo, qabs[(bh * ncq + c) * 2 + 1]);
    }
  }
  const int ek = nos::h3_scale_exp(mk), eq = nos::h3_scale_exp(mq), edo = nos::h3_scale_exp(mdo);
  int eds = 0;  // (2 scale D max|dO| max|V|) 2^eds < 2^14
  if (mdo > 0.f && mv > 0.f) {
    eds = 14 - (ub_exp(mdo) + ub_exp(mv) + ub_exp(2.f * scale * (float)D));
    eds = eds < -100 ? -100 : (eds > 100 ? 100 : eds);
  }
  const int ev = nos::h3_scale_exp(mv);
  float* o = grp + (long long)i * GRP;
  o[G_QSC] = nos::pow2i(eq);
  o[G_DOSC] = nos::pow2i(edo);
  o[G_A1] = ldexpf(scale, eds - (int)P_EXP - edo - ev);  // dS' = P' (dP' a1 - delta a2)
  o[G_A2] = ldexpf(scale, eds - (int)P_EXP);
  o[G_DVF] = ldexpf(1.f, -(int)P_EXP - edo);
  o[G_DKF] = ldexpf(1.f, -eds - eq);
  o[G_DQF] = ldexpf(1.f, -eds - ek);
  o[G_KINV] = nos::pow2i(-ek);
}

// ---------------------------------------------------------------- Q / dO rows
// D / 8 threads per query row (b, h, s < sqp): row planes
// qrows[(bh * sqp + s) * 4 + {Q hi, Q lo, dO hi, dO lo}][D] -- Q on the
// forward's per-row scale (softmax scale folded in), dO on its group scale --
// and rinfo[bh * sqp + s] = {2^-e_row, -lse log2 e (hi), 13 - (lo), delta}.
// Rows s >= Sq: zero planes and finite constants.
template <int D>
__global__ __launch_bounds__(256) void bwd_rows_kernel(const float* __restrict__ q, int ldq, long long bsq,
                                                       const float* __restrict__ o, int ldo, long long bso,
                                                       const float* __restrict__ dout, int lddo, long long bsdo,
                                                       const float* __restrict__ lse, const float* __restrict__ grp,
                                                       _Float16* __restrict__ qrows, float4* __restrict__ rinfo,
                                                       int H, int Hkv, int Sq, int sqp, float c, long long nrows) {
  constexpr int TPR = D / 8;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = gid / TPR;
  const int ch = (int)(gid - row * TPR);
  const bool live_row = row < nrows;   // whole TPR-lane groups are in or out together
  const long long rw = live_row ? row : nrows - 1;
  const int s = (int)(rw % sqp);
  const long long bh = rw / sqp;
  const int b = (int)(bh / H), h = (int)(bh - (long long)b * H);
  const bool real = s < Sq;
  float x[8], y[8], z[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = y[j] = z[j] = 0.f;
  if (real) {
    const float* qp = q + b * bsq + (long long)s * ldq + h * D + ch * 8;
    const float* op = o + b * bso + (long long)s * ldo + h * D + ch * 8;
    const float* dp = dout + b * bsdo + (long long)s * lddo + h * D + ch * 8;
    const float4 a0 = *reinterpret_cast<const float4*>(qp), a1 = *reinterpret_cast<const float4*>(qp + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(op), b1 = *reinterpret_cast<const float4*>(op + 4);
    const float4 c0 = *reinterpret_cast<const float4*>(dp), c1 = *reinterpret_cast<const float4*>(dp + 4);
    x[0] = a0.x; x[1] = a0.y; x[2] = a0.z; x[3] = a0.w; x[4] = a1.x; x[5] = a1.y; x[6] = a1.z; x[7] = a1.w;
    y[0] = b0.x; y[1] = b0.y; y[2] = b0.z; y[3] = b0.w; y[4] = b1.x; y[5] = b1.y; y[6] = b1.z; y[7] = b1.w;
    z[0] = c0.x; z[1] = c0.y; z[2] = c0.z; z[3] = c0.w; z[4] = c1.x; z[5] = c1.y; z[6] = c1.z; z[7] = c1.w;
  }
  float mx = 0.f, dl = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mx = fmaxf(mx, fabsf(x[j]));
    dl = fmaf(z[j], y[j], dl);
  }
#pragma unroll
  for (int m = TPR / 2; m > 0; m >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    dl += __shfl_xor(dl, m, 64);
  }
  if (!live_row) return;
  const int e = nos::h3_scale_exp(mx * c);   // the forward's Q scale
  const float qm = c * nos::pow2i(e);
  const float dosc = grp[((long long)b * Hkv + h / (H / Hkv)) * GRP + G_DOSC];
  f16x8_t qh, ql, dh, dlo;
  nos::split8h(x, qm, qh, ql);
  nos::split8h(z, dosc, dh, dlo);
  _Float16* dst = qrows + rw * 4 * D + ch * 8;
  *reinterpret_cast<f16x8_t*>(dst) = qh;
  *reinterpret_cast<f16x8_t*>(dst + D) = ql;
  *reinterpret_cast<f16x8_t*>(dst + 2 * D) = dh;
  *reinterpret_cast<f16x8_t*>(dst + 3 * D) = dlo;
  if (ch == 0) {
    float4 ri = {1.f, 0.f, P_EXP, 0.f};
    if (real) {
      const float l = lse[bh * Sq + s];
      const float L2E = 1.4426950408889634f, L2E_LO = 1.9259629911e-8f;  // log2 e = L2E + L2E_LO
      const float hi = l * L2E;
      const float lo = fmaf(l, L2E, -hi) + l * L2E_LO;
      ri = float4{nos::pow2i(-e), -hi, P_EXP - lo, dl};
    }
    rinfo[rw] = ri;
  }
}

// ---------------------------------------------------------------- transposed planes
// x [B, S, Hx, D] (ld, bs) as tp[((bh * nt + tile) * np + p0 + piece) * D + d][32 rows]
// on the scale scl[(b * (Hx / sdiv) + h / sdiv) * sstride + soff]; one thread:
// 8 rows of one d (lanes run over d: coalesced reads); rows >= S are zeros
__global__ __launch_bounds__(256) void bwd_tsplit_kernel(const float* __restrict__ x, int ld, long long bs,
                                                         const float* __restrict__ scl, int sdiv, int sstride,
                                                         int soff, _Float16* __restrict__ tp, int np, int p0, int S,
                                                         int nt, int Hx, int D, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i % D);
  long long rest = i / D;
  const int cq = (int)(rest & 3);
  rest >>= 2;
  const int tile = (int)(rest % nt);
  const long long bh = rest / nt;
  const int b = (int)(bh / Hx), h = (int)(bh - (long long)b * Hx);
  const float sc = scl[((long long)b * (Hx / sdiv) + h / sdiv) * sstride + soff];
  const int s0 = tile * 32 + cq * 8;
  const float* src = x + b * bs + h * D + d;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = s0 + j < S ? src[(long long)(s0 + j) * ld] * sc : 0.f;
  f16x8_t hi, lo;
  nos::split8h(v, 1.f, hi, lo);
  _Float16* dst = tp + ((((long long)bh * nt + tile) * np + p0) * D + d) * 32 + cq * 8;
  *reinterpret_cast<f16x8_t*>(dst) = hi;
  *reinterpret_cast<f16x8_t*>(dst + (long long)D * 32) = lo;
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;   // a 16-byte chunk in flight

// LDS images (bytes): row planes [plane][32 rows][D + 8], transposed planes
// [plane][D][TP], the tile's per-row constants.  A tile is staged as 16-byte
// chunks, chunk tid + 256 i in register i of the 256 threads; row_off / t_off
// place a chunk in the image (the stores stay in the kernels: docs/status.md)
template <int D>
struct Img {
  static constexpr int RS = (D + 8) * 2;       // row stride of a row plane
  static constexpr int ROWS = 4 * 32 * RS;     // four row planes
  static constexpr int TS = TP * 2;            // row stride of a transposed plane
  static constexpr int NR = D / 16;            // 16-byte chunks per thread: four row planes of a tile

  // chunk cidx of a tile's four row planes ([row][plane][D] in global memory)
  static __device__ __forceinline__ int row_off(int cidx) {
    const int row = cidx / (D / 2), within = cidx % (D / 2);      // 4 D / 8 chunks per row
    const int plane = within / (D / 8), ch = within % (D / 8);
    return (plane * 32 + row) * RS + ch * 16;
  }
  // chunk cidx of a tile's transposed planes, from the first plane's start
  static __device__ __forceinline__ int t_off(int cidx) { return (cidx >> 2) * TS + (cidx & 3) * 16; }
};

__device__ __forceinline__ f16x8_t lds16(const unsigned char* p) { return *reinterpret_cast<const f16x8_t*>(p); }

// A operand of a product that reduces over rows: the rows 16 s2 + 4 hh +
// {0..3, 8..11} of column (lane & 31) of a transposed plane -- the order in
// which a lane holds a 32x32 accumulator's values as the B operand
__device__ __forceinline__ f16x8_t lds_t(const unsigned char* p) {
  const s16x4_t lo4 = *reinterpret_cast<const s16x4_t*>(p);
  const s16x4_t hi4 = *reinterpret_cast<const s16x4_t*>(p + 16);
  const s16x8_t a = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
  return __builtin_bit_cast(f16x8_t, a);
}

// ---------------------------------------------------------------- dK, dV
template <int D, bool CAUSAL>
__global__ __launch_bounds__(64 * BW, 1) void attn_h3g_bwd_dkdv_kernel(
    const _Float16* __restrict__ kvs, const _Float16* __restrict__ qrows, const _Float16* __restrict__ qT,
    const float4* __restrict__ rinfo, const float* __restrict__ grp, float* __restrict__ dk, int lddk,
    long long bsdk, float* __restrict__ dv, int lddv, long long bsdv, float* __restrict__ part, int B, int H, int Hkv,
    int Sq, int Skv, int nkb, int nsplit) {
  using L = Img<D>;
  constexpr int NKS = D / 16, NDB = D / 32, NR = L::NR;
  constexpr int TOFF = L::ROWS, IOFF = L::ROWS + 4 * D * L::TS;
  // each wave's V B-operands, in register order ([step][piece][lane] x 16 bytes): K's stay in
  // registers, both would leave the arch-VGPR half too small for the tiles in flight
  constexpr int VOFF = IOFF + 32 * 16, VWAVE = NKS * 2 * 1024;
  __shared__ __attribute__((aligned(16))) unsigned char smem[VOFF + BW * VWAVE];

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r = lane & 31, hh = lane >> 5;
  unsigned char* const vlds = smem + VOFF + wid * VWAVE + lane * 16;   // wave-private: no barrier
  const int g = H / Hkv;
  const int ntq = (Sq + 31) / 32, sqp = ntq * 32;
  const int skvp = padded_keys(Skv);
  const int off = Skv - Sq;
  const nos::XcdChunk chunk = nos::xcd_chunk(blockIdx.x, gridDim.x, B * Hkv * nkb * nsplit);

  for (int w = chunk.first; w < chunk.end; w += chunk.step) {
    if (w != chunk.first) __syncthreads();
    const int sp = w % nsplit;
    const int wk = w / nsplit;
    const int b = wk / (Hkv * nkb);
    const int rem = wk - b * (Hkv * nkb);
    const int hk = rem / nkb;
    const int kb = rem - hk * nkb;          // causal: early key blocks see the most queries, and come first
    const int k0 = kb * BLK, kw0 = k0 + wid * 32;
    const int qt_first = CAUSAL ? max(0, k0 - off) / 32 : 0;
    const int ntl = ntq - qt_first;
    const int ntot = g * ntl;
    const int per = (ntot + nsplit - 1) / nsplit;
    const int n0 = sp * per, n1 = min(ntot, n0 + per);
    const float* gp = grp + (long long)(b * Hkv + hk) * GRP;
    const float kinv = gp[G_KINV], a1 = gp[G_A1], a2 = gp[G_A2];

    // this wave's keys as B operands, for the whole sweep
    const int key = kw0 + r;
    f16x8_t kf[NKS][2];
    {
      const _Float16* kp = kvs + ((long long)(b * Hkv + hk) * skvp + min(key, Skv - 1)) * 4 * D + 8 * hh;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          kf[ks][pc] = *reinterpret_cast<const f16x8_t*>(kp + pc * D + 16 * ks);
          *reinterpret_cast<f16x8_t*>(vlds + (ks * 2 + pc) * 1024) =
              *reinterpret_cast<const f16x8_t*>(kp + (2 + pc) * D + 16 * ks);
        }
    }
    f32x16_t dkacc[NDB], dvacc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) dkacc[db][i] = dvacc[db][i] = 0.f;

    // Staging in two halves so that only one is in flight in registers: the
    // row planes (+ row constants) feed S / dP, the transposed planes feed
    // dV^T / dK^T; each half's LDS image is rewritten once every wave is past
    // the phase that reads it.
    u32x4_t rr[NR];
    f32x4_t inf = {1.f, 0.f, P_EXP, 0.f};
    auto tile_of = [&](int n, long long& bh, int& qt) {
      const int hg = n / ntl;
      qt = qt_first + (n - hg * ntl);
      bh = (long long)b * H + hk * g + hg;
    };
    auto fetch_rows = [&](int n) {
      long long bh;
      int qt;
      tile_of(n, bh, qt);
      const u32x4_t* rs = reinterpret_cast<const u32x4_t*>(qrows + (bh * sqp + qt * 32) * 4 * D);
#pragma unroll
      for (int i = 0; i < NR; ++i) rr[i] = rs[tid + 256 * i];
      if (tid < 32) inf = *reinterpret_cast<const f32x4_t*>(rinfo + bh * sqp + qt * 32 + tid);
    };
    auto fetch_t = [&](int n) {
      long long bh;
      int qt;
      tile_of(n, bh, qt);
      const u32x4_t* ts = reinterpret_cast<const u32x4_t*>(qT + (bh * ntq + qt) * 4 * D * 32);
#pragma unroll
      for (int i = 0; i < NR; ++i) rr[i] = ts[tid + 256 * i];
    };
    auto store_rows = [&]() {
#pragma unroll
      for (int i = 0; i < NR; ++i) *reinterpret_cast<u32x4_t*>(smem + L::row_off(tid + 256 * i)) = rr[i];
      if (tid < 32) *reinterpret_cast<f32x4_t*>(smem + IOFF + tid * 16) = inf;
    };
    auto store_t = [&]() {
#pragma unroll
      for (int i = 0; i < NR; ++i) *reinterpret_cast<u32x4_t*>(smem + TOFF + L::t_off(tid + 256 * i)) = rr[i];
    };

    if (n0 < n1) {
      fetch_rows(n0);
      store_rows();
      fetch_t(n0);
      store_t();
    }
    __syncthreads();
    for (int n = n0; n < n1; ++n) {
      const int nn = min(n + 1, n1 - 1);   // the last iteration re-reads its own tile: no branch around the registers in flight
      fetch_rows(nn);
      const int qt0 = (qt_first + n % ntl) * 32;
      // no wave-uniform skip of masked tiles: a branch around the MFMAs makes the register allocator keep two
      // copies of the dK^T / dV^T accumulators (spills at head_dim 128); the masks below zero what is not seen
      f16x8_t pf[2][2], sf[2][2];
      {
        // S, then P; dP, then dS: one 32x32 accumulator at a time beside dK^T / dV^T
        f32x16_t s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const unsigned char* base = smem + r * L::RS + (16 * ks + 8 * hh) * 2;
          const f16x8_t qh = lds16(base), ql = lds16(base + 32 * L::RS);
          // the forward's order: K lo . Q hi, K hi . Q lo, K hi . Q hi
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh, kf[ks][1], s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ql, kf[ks][0], s, 0, 0, 0);
          s = __builtin_amdgcn_mfma_f32_32x32x16_f16(qh, kf[ks][0], s, 0, 0, 0);
        }
        // acc i: query qt0 + (i & 3) + 8 (i >> 2) + 4 hh, key = this lane's
#pragma unroll
        for (int j2 = 0; j2 < 8; ++j2) {
          float p2[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int i = 2 * j2 + u;
            const int qloc = (i & 3) + 8 * (i >> 2) + 4 * hh;
            const float4 ri = *reinterpret_cast<const float4*>(smem + IOFF + qloc * 16);
            const int qq = qt0 + qloc;
            const bool ok = key < Skv && qq < Sq && (!CAUSAL || key <= qq + off);
            const float x = fmaf(s[i], ri.x * kinv, ri.y) + ri.z;
            p2[u] = ok ? __builtin_amdgcn_exp2f(x) : 0.f;
            s[i] = p2[u];
          }
          nos::set_pair(pf, j2, f32x2_t{p2[0], p2[1]});
        }
        f32x16_t dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const unsigned char* base = smem + (64 + r) * L::RS + (16 * ks + 8 * hh) * 2;
          const f16x8_t da[2] = {lds16(base), lds16(base + 32 * L::RS)};
          const f16x8_t vb[2] = {lds16(vlds + ks * 2048), lds16(vlds + ks * 2048 + 1024)};
          dp = nos::mma3h(da, vb, dp);
        }
#pragma unroll
        for (int j2 = 0; j2 < 8; ++j2) {
          float d2[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int i = 2 * j2 + u;
            const int qloc = (i & 3) + 8 * (i >> 2) + 4 * hh;
            const float delta = *reinterpret_cast<const float*>(smem + IOFF + qloc * 16 + 12);
            d2[u] = s[i] * fmaf(dp[i], a1, -delta * a2);
          }
          nos::set_pair(sf, j2, f32x2_t{d2[0], d2[1]});
        }
      }
      __syncthreads();   // every wave is past the row planes of tile n
      store_rows();
      fetch_t(nn);
      {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const unsigned char* base = smem + TOFF + (32 * db + r) * L::TS + (16 * s2 + 4 * hh) * 2;
            const f16x8_t qa[2] = {lds_t(base), lds_t(base + D * L::TS)};
            const f16x8_t da[2] = {lds_t(base + 2 * D * L::TS), lds_t(base + 3 * D * L::TS)};
            dvacc[db] = nos::mma3h(da, pf[s2], dvacc[db]);   // dV^T += dO^T P
            dkacc[db] = nos::mma3h(qa, sf[s2], dkacc[db]);   // dK^T += Q^T dS
          }
      }
      __syncthreads();   // every wave is past the transposed planes of tile n; the next row planes are published
      store_t();         // published by the next iteration's first barrier (or the item loop's)
    }

    // acc [db][4 gq + j]: d = 32 db + 8 gq + 4 hh + j of key `key`
    const float dkf = gp[G_DKF], dvf = gp[G_DVF];
    if (key < Skv) {
      float *pk, *pv;
      if (nsplit == 1) {
        pk = dk + b * bsdk + (long long)key * lddk + hk * D;
        pv = dv + b * bsdv + (long long)key * lddv + hk * D;
      } else {
        pk = part + ((((long long)sp * B + b) * Skv + key) * Hkv + hk) * 2 * D;
        pv = pk + D;
      }
      // not nos::store_acc32: dK's four stores of a block before dV's reorders the epilogue (docs/status.md)
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int d = 32 * db + 8 * gq + 4 * hh;
          *reinterpret_cast<float4*>(pk + d) = float4{dkacc[db][4 * gq] * dkf, dkacc[db][4 * gq + 1] * dkf,
                                                      dkacc[db][4 * gq + 2] * dkf, dkacc[db][4 * gq + 3] * dkf};
          *reinterpret_cast<float4*>(pv + d) = float4{dvacc[db][4 * gq] * dvf, dvacc[db][4 * gq + 1] * dvf,
                                                      dvacc[db][4 * gq + 2] * dvf, dvacc[db][4 * gq + 3] * dvf};
        }
    }
  }  // items
}

// the ranges of a split sweep, added in order: part[sp][b][key][hk][dK | dV][D]
__global__ __launch_bounds__(256) void bwd_merge_kernel(const float* __restrict__ part, float* __restrict__ dk,
                                                        int lddk, long long bsdk, float* __restrict__ dv, int lddv,
                                                        long long bsdv, int B, int Hkv, int Skv, int D, int nsplit,
                                                        long long n4) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c4 = (int)(i % (2 * D / 4)) * 4;
  long long rest = i / (2 * D / 4);
  const int hk = (int)(rest % Hkv);
  rest /= Hkv;
  const int key = (int)(rest % Skv);
  const int b = (int)(rest / Skv);
  const long long per = (long long)B * Skv * Hkv * 2 * D;
  const float* p = part + i * 4;
  float4 acc = *reinterpret_cast<const float4*>(p);
  for (int sp = 1; sp < nsplit; ++sp) {
    const float4 v = *reinterpret_cast<const float4*>(p + sp * per);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  float* dst = c4 < D ? dk + b * bsdk + (long long)key * lddk + hk * D + c4
                      : dv + b * bsdv + (long long)key * lddv + hk * D + (c4 - D);
  *reinterpret_cast<float4*>(dst) = acc;
}

// ---------------------------------------------------------------- dQ
template <int D, bool CAUSAL>
__global__ __launch_bounds__(64 * BW, 1) void attn_h3g_bwd_dq_kernel(
    const _Float16* __restrict__ kvs, const _Float16* __restrict__ kT, const _Float16* __restrict__ qrows,
    const float4* __restrict__ rinfo, const float* __restrict__ grp, float* __restrict__ dq, int lddq,
    long long bsdq, int B, int H, int Hkv, int Sq, int Skv, int nqb) {
  using L = Img<D>;
  constexpr int NKS = D / 16, NDB = D / 32, NR = L::NR, NT = D / 32;
  constexpr int TOFF = L::ROWS;
  __shared__ __attribute__((aligned(16))) unsigned char smem[TOFF + 2 * D * L::TS];

  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, r = lane & 31, hh = lane >> 5;
  const int g = H / Hkv;
  const int sqp = (Sq + 31) / 32 * 32;
  const int skvp = padded_keys(Skv), ntk = skvp / KVB;
  const int off = Skv - Sq;
  const nos::XcdChunk chunk = nos::xcd_chunk(blockIdx.x, gridDim.x, B * H * nqb);

  for (int w = chunk.first; w < chunk.end; w += chunk.step) {
    if (w != chunk.first) __syncthreads();
    const int b = w / (H * nqb);
    const int rem = w - b * (H * nqb);
    const int h = rem / nqb;
    const int qb = CAUSAL ? nqb - 1 - (rem - h * nqb) : rem - h * nqb;   // causal: the longest rows first
    const int hk = h / g;
    const int q0 = qb * BLK, qw0 = q0 + wid * 32;
    const int qrow = qw0 + r;
    const int nt = CAUSAL ? min(ntk, (min(q0 + BLK, Sq) - 1 + off) / KVB + 1) : ntk;
    const float* gp = grp + (long long)(b * Hkv + hk) * GRP;
    const float a1 = gp[G_A1];
    const long long bh = (long long)b * H + h;
    const long long qr = bh * sqp + min(qrow, Sq - 1);

    // this wave's query rows as B operands, for the whole sweep
    f16x8_t qf[NKS][2], dof[NKS][2];
    {
      const _Float16* qp = qrows + qr * 4 * D + 8 * hh;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          qf[ks][pc] = *reinterpret_cast<const f16x8_t*>(qp + pc * D + 16 * ks);
          dof[ks][pc] = *reinterpret_cast<const f16x8_t*>(qp + (2 + pc) * D + 16 * ks);
        }
    }
    const float4 ri = rinfo[qr];
    const float fs = ri.x * gp[G_KINV], nh = ri.y, c13 = ri.z, da2 = ri.w * gp[G_A2];
    f32x16_t dqacc[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) dqacc[db][i] = 0.f;

    const _Float16* kvb = kvs + (long long)(b * Hkv + hk) * skvp * 4 * D;
    const _Float16* ktb = kT + (long long)(b * Hkv + hk) * ntk * 2 * D * 32;
    u32x4_t rr[NR], tt[NT];
    auto fetch = [&](int t) {
#pragma unroll
      for (int i = 0; i < NR; ++i) {
        const int cidx = tid + 256 * i;
        const int row = min(t * KVB + cidx / (D / 2), Skv - 1);   // rows past Skv re-read the last key (masked)
        rr[i] = *reinterpret_cast<const u32x4_t*>(kvb + (long long)row * 4 * D + (cidx % (D / 2)) * 8);
      }
      const u32x4_t* ts = reinterpret_cast<const u32x4_t*>(ktb + (long long)t * 2 * D * 32);
#pragma unroll
      for (int i = 0; i < NT; ++i) tt[i] = ts[tid + 256 * i];
    };
    auto store = [&]() {
#pragma unroll
      for (int i = 0; i < NR; ++i) *reinterpret_cast<u32x4_t*>(smem + L::row_off(tid + 256 * i)) = rr[i];
#pragma unroll
      for (int i = 0; i < NT; ++i) *reinterpret_cast<u32x4_t*>(smem + TOFF + L::t_off(tid + 256 * i)) = tt[i];
    };

    fetch(0);
    store();
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      fetch(min(t + 1, nt - 1));   // the last iteration re-reads its own tile: no branch around the registers in flight
      {   // no wave-uniform skip of masked tiles (see the dK / dV kernel)
        f32x16_t s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
          const unsigned char* base = smem + r * L::RS + (16 * ks + 8 * hh) * 2;
          const f16x8_t ka[2] = {lds16(base), lds16(base + 32 * L::RS)};
          const f16x8_t va[2] = {lds16(base + 64 * L::RS), lds16(base + 96 * L::RS)};
          s = nos::mma3h(ka, qf[ks], s);      // S^T = K Q^T, the forward's pieces and order
          dp = nos::mma3h(va, dof[ks], dp);   // dP^T = V dO^T
        }
        // acc i: key t KVB + (i & 3) + 8 (i >> 2) + 4 hh, query = this lane's
        f16x8_t sf[2][2];
#pragma unroll
        for (int j2 = 0; j2 < 8; ++j2) {
          float d2[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int i = 2 * j2 + u;
            const int kk = t * KVB + (i & 3) + 8 * (i >> 2) + 4 * hh;
            const bool ok = kk < Skv && qrow < Sq && (!CAUSAL || kk <= qrow + off);
            const float x = fmaf(s[i], fs, nh) + c13;
            const float p = ok ? __builtin_amdgcn_exp2f(x) : 0.f;
            d2[u] = p * fmaf(dp[i], a1, -da2);
          }
          nos::set_pair(sf, j2, f32x2_t{d2[0], d2[1]});
        }
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const unsigned char* base = smem + TOFF + (32 * db + r) * L::TS + (16 * s2 + 4 * hh) * 2;
            const f16x8_t ka[2] = {lds_t(base), lds_t(base + D * L::TS)};
            dqacc[db] = nos::mma3h(ka, sf[s2], dqacc[db]);   // dQ^T += K^T dS^T
          }
      }
      __syncthreads();
      store();
      __syncthreads();
    }

    const float dqf = gp[G_DQF];
    if (qrow < Sq) {
      float* p = dq + b * bsdq + (long long)qrow * lddq + h * D;
#pragma unroll
      for (int db = 0; db < NDB; ++db) nos::store_acc32(p + 32 * db, dqacc[db], dqf, hh);
    }
  }  // items
}

struct Layout {
  long long kvs, kT, qrows, qT, rinfo, kvabs, qabs, kvsc, grp, part, total;
  int skvp, sqp;
};

Layout layout(int B, int H, int Hkv, int Sq, int Skv, int D) {
  Layout L;
  L.skvp = padded_keys(Skv);
  L.sqp = (Sq + 31) / 32 * 32;
  L.kvs = 0;
  L.kT = align256((long long)B * Hkv * L.skvp * 4 * D * 2);
  L.qrows = L.kT + align256((long long)B * Hkv * L.skvp * 2 * D * 2);
  L.qT = L.qrows + align256((long long)B * H * L.sqp * 4 * D * 2);
  L.rinfo = L.qT + align256((long long)B * H * L.sqp * 4 * D * 2);
  L.kvabs = L.rinfo + align256((long long)B * H * L.sqp * 16);
  L.qabs = L.kvabs + align256((long long)B * Hkv * abs_chunks(Skv) * 2 * 4);
  L.kvsc = L.qabs + align256((long long)B * H * abs_chunks(Sq) * 2 * 4);
  L.grp = L.kvsc + align256((long long)B * Hkv * 2 * 4);
  L.part = L.grp + align256((long long)B * Hkv * GRP * 4);
  L.total = L.part + (long long)MAX_QSPLIT * B * Skv * Hkv * 2 * D * 4;
  return L;
}

// what the main launches take: the workspace sections, the gradients, the shape
struct BwdCall {
  const _Float16 *kvs, *kT, *qrows, *qT;
  const float4* rinfo;
  const float* grp;
  float *dq, *dk, *dv, *part;
  int lddq, lddk, lddv;
  long long bsdq, bsdk, bsdv;
  int B, H, Hkv, Sq, Skv;
};

template <int D, bool CAUSAL>
int launch_main(const BwdCall& c, hipStream_t stream) {
  const int nkb = (c.Skv + BLK - 1) / BLK, nqb = (c.Sq + BLK - 1) / BLK;
  const long long items1 = (long long)c.B * c.Hkv * nkb;
  // ranges of the query sweep while the grid leaves CUs idle (each range keeps at least ~4 tiles)
  const long long slots = nos_effective_cus();
  int nsplit = items1 >= slots ? 1 : (int)(slots / items1);
  const int ntot = (c.H / c.Hkv) * ((c.Sq + 31) / 32);
  nsplit = nsplit > MAX_QSPLIT ? MAX_QSPLIT : nsplit;
  while (nsplit > 1 && ntot / nsplit < 4) --nsplit;
  const long long items = items1 * nsplit;
  const int grid = nos_grid_for((const void*)attn_h3g_bwd_dkdv_kernel<D, CAUSAL>, 64 * BW, 0, items);
  hipLaunchKernelGGL((attn_h3g_bwd_dkdv_kernel<D, CAUSAL>), dim3((unsigned)grid), dim3(64 * BW), 0, stream, c.kvs,
                     c.qrows, c.qT, c.rinfo, c.grp, c.dk, c.lddk, c.bsdk, c.dv, c.lddv, c.bsdv, c.part, c.B, c.H, c.Hkv,
                     c.Sq, c.Skv, nkb, nsplit);
  if (int rc = (int)hipGetLastError()) return rc;
  if (nsplit > 1) {
    const long long n4 = (long long)c.B * c.Skv * c.Hkv * 2 * D / 4;
    hipLaunchKernelGGL(bwd_merge_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, c.part, c.dk, c.lddk,
                       c.bsdk, c.dv, c.lddv, c.bsdv, c.B, c.Hkv, c.Skv, D, nsplit, n4);
  }
  const long long qitems = (long long)c.B * c.H * nqb;
  const int qgrid = nos_grid_for((const void*)attn_h3g_bwd_dq_kernel<D, CAUSAL>, 64 * BW, 0, qitems);
  hipLaunchKernelGGL((attn_h3g_bwd_dq_kernel<D, CAUSAL>), dim3((unsigned)qgrid), dim3(64 * BW), 0, stream, c.kvs, c.kT,
                     c.qrows, c.rinfo, c.grp, c.dq, c.lddq, c.bsdq, c.B, c.H, c.Hkv, c.Sq, c.Skv, nqb);
  return (int)hipGetLastError();
}

}  // namespace

// Workspace bytes of nos_attn_h3g_bwd (planes, constants, partial dK / dV of a split sweep).
NOS_API long long nos_attn_h3g_bwd_workspace(int B, int H, int Hkv, int Sq, int Skv, int D) {
  if (!attn_dims_ok(B, H, Hkv, Sq, Skv, D) || H % Hkv) return -1;
  return layout(B, H, Hkv, Sq, Skv, D).total;
}

// dq, dk, dv of nos_attn_h3g_lse's O = softmax(scale Q K^T [causal]) V: fp32
// q, o, dO [B, Sq, H, D], k, v [B, Skv, Hkv, D] (token row strides ld*, batch
// strides bs*, each head's D dims contiguous), lse [B][H][Sq] from the
// forward; dq / dk / dv in the shapes of q / k / v.  D = 64 or 128,
// H % Hkv == 0, causal needs Sq <= Skv; no rotary (rotate in a node of its
// own).  ws: at least nos_attn_h3g_bwd_workspace() bytes, 256-byte aligned.
// Every launch goes to `stream`; nothing is allocated, synchronised or read
// back, so the call can be captured into a graph.
NOS_API int nos_attn_h3g_bwd(const float* q, int ldq, long long bsq, const float* k, int ldk, long long bsk,
                             const float* v, int ldv, long long bsv, const float* o, int ldo, long long bso,
                             const float* dout, int lddo, long long bsdo, const float* lse, float* dq, int lddq,
                             long long bsdq, float* dk, int lddk, long long bsdk, float* dv, int lddv, long long bsdv,
                             int B, int H, int Hkv, int Sq, int Skv, int D, int causal, float scale, void* ws,
                             long long ws_bytes, hipStream_t stream) {
  const Rows Q{q, ldq, bsq}, K{k, ldk, bsk}, V{v, ldv, bsv}, O{o, ldo, bso}, DO{dout, lddo, bsdo};
  if (!attn_call_ok(B, H, Hkv, Sq, Skv, D, causal, scale, ws, ws_bytes, nos_attn_h3g_bwd_workspace) ||
      !Q.ok(H, D) || !O.ok(H, D) || !DO.ok(H, D) || !Rows{dq, lddq, bsdq}.ok(H, D) || !K.ok(Hkv, D) ||
      !V.ok(Hkv, D) || !Rows{dk, lddk, bsdk}.ok(Hkv, D) || !Rows{dv, lddv, bsdv}.ok(Hkv, D))
    return (int)hipErrorInvalidValue;
  if (lse == nullptr || ((uintptr_t)lse & 3)) return (int)hipErrorInvalidValue;
  const Layout L = layout(B, H, Hkv, Sq, Skv, D);
  if ((long long)B * H * L.sqp * 4 * D > INT_MAX * 8LL || (long long)B * Hkv * L.skvp * 4 * D > INT_MAX * 8LL ||
      (long long)B * H * ((Sq + 31) / 32 + (Skv + 31) / 32) * MAX_QSPLIT > (1LL << 30))
    return (int)hipErrorInvalidValue;
  auto* base = static_cast<unsigned char*>(ws);
  auto* kvs = reinterpret_cast<_Float16*>(base + L.kvs);
  auto* kT = reinterpret_cast<_Float16*>(base + L.kT);
  auto* qrows = reinterpret_cast<_Float16*>(base + L.qrows);
  auto* qT = reinterpret_cast<_Float16*>(base + L.qT);
  auto* rinfo = reinterpret_cast<float4*>(base + L.rinfo);
  auto* kvabs = reinterpret_cast<float*>(base + L.kvabs);
  auto* qabs = reinterpret_cast<float*>(base + L.qabs);
  auto* kvsc = reinterpret_cast<float*>(base + L.kvsc);
  auto* grp = reinterpret_cast<float*>(base + L.grp);
  const int nbk = B * Hkv, nbq = B * H, g = H / Hkv;
  const float c = scale * nos::LOG2E;
  auto blocks = [](long long n) { return dim3((unsigned)((n + 255) / 256)); };

  // K / V as the forward sees them; Q / dO maxima through the same kernel (H heads of Sq rows)
  launch_kv_prepass(K, V, kvabs, kvsc, kvs, B, Hkv, Skv, D, 1.f, nullptr, nullptr, stream);
  launch_absmax(Q, DO, qabs, nbq, Sq, H, D, stream);
  hipLaunchKernelGGL(bwd_scale_kernel, blocks(nbk), dim3(256), 0, stream, kvabs, qabs, grp, nbk, Hkv, g,
                     abs_chunks(Skv), abs_chunks(Sq), scale, D);
  const long long nrows = (long long)nbq * L.sqp;
  hipLaunchKernelGGL(D == 64 ? bwd_rows_kernel<64> : bwd_rows_kernel<128>, blocks(nrows * (D / 8)), dim3(256), 0,
                     stream, q, ldq, bsq, o, ldo, bso, dout, lddo, bsdo, lse, grp, qrows, rinfo, H, Hkv, Sq, L.sqp, c,
                     nrows);
  const int ntk = L.skvp / 32, ntq = L.sqp / 32;
  const long long nk = (long long)nbk * ntk * 4 * D, nq = (long long)nbq * ntq * 4 * D;
  hipLaunchKernelGGL(bwd_tsplit_kernel, blocks(nk), dim3(256), 0, stream, k, ldk, bsk, kvsc, 1, 2, 0, kT, 2, 0, Skv, ntk,
                     Hkv, D, nk);
  hipLaunchKernelGGL(bwd_tsplit_kernel, blocks(nq), dim3(256), 0, stream, q, ldq, bsq, grp, g, GRP, (int)G_QSC, qT, 4, 0,
                     Sq, ntq, H, D, nq);
  hipLaunchKernelGGL(bwd_tsplit_kernel, blocks(nq), dim3(256), 0, stream, dout, lddo, bsdo, grp, g, GRP, (int)G_DOSC, qT,
                     4, 2, Sq, ntq, H, D, nq);
  if (int rc = (int)hipGetLastError()) return rc;
  const BwdCall call{kvs, kT, qrows, qT, rinfo, grp, dq, dk, dv, reinterpret_cast<float*>(base + L.part), lddq, lddk,
                     lddv, bsdq, bsdk, bsdv, B, H, Hkv, Sq, Skv};
  const auto run = D == 64 ? (causal ? launch_main<64, true> : launch_main<64, false>)
                           : (causal ? launch_main<128, true> : launch_main<128, false>);
  return run(call, stream);
}
