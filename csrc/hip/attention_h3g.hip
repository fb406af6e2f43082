// General fp32 attention on the fp16x3 ("h3") matrix pipes: the attention of
// tenant programs that are not ViT encoders -- decoder LLMs (causal, head_dim
// 128, grouped-query K/V heads, rotary position embeddings), and any
// head_dim-64 attention whose K / V are not the output of a fused LN-QKV GEMM.
//
//   O = softmax(scale Q K^T [+ causal mask]) V,   q / k / v fp32 [B, S, H(kv), D]
//
// Same numerics as the YOLOS h3 kernel (attention_f32x.hip; split_f16.h):
// every operand is two fp16 pieces on a power-of-two scale and every product
// the three piece products ah.bh + ah.bl + al.bh on v_mfma_f32_32x32x16_f16
// (22 of an fp32's 24 bits, fp32 accumulation), within the exact-f32
// kernel's error against fp64 (tests/test_tenant_ops_gpu.py).  What differs
// is where the K / V scales come from: here K / V are arbitrary activations,
// so a pre-pass (attn_kv_planes.h, shared with the backward) measures them --
//
//  1. kv_absmax: max |k| and |v| per (batch, kv head) over row chunks;
//  2. kv_scale: the power of two that puts each head's max just under 2^14
//     (for rotated keys: the host's bound max|cos| + max|sin| on top);
//  3. split_kv: K (rotated on the fly) and V as four fp16 planes per token,
//     [b][kv head][token][K hi, K lo, V hi, V lo][D], 16-byte stores;
//  4. the attention: one workgroup = 8 waves x 32 query rows of one (batch,
//     head); 32-key tiles of the four planes arrive by LDS-DMA
//     (global_load_lds_dwordx4) into a 2-deep ring, each 64-dim half of a
//     plane as its own XOR-swizzled 4 KiB image (head_dim 128 = two halves
//     of the head_dim-64 layout); swapped S^T = K Q^T with Q's pieces (its
//     per-row scale and the softmax scale folded in, rotated on load) in
//     registers; P = exp2(S - m) split in registers and fed straight to
//     O^T = V^T P^T through ds_read_b64_tr_b16; deferred rescale (P <= 2^8);
//     causal tiles past a workgroup's last query are never loaded, the
//     diagonal tiles masked per lane, heavy (late) query blocks first;
//     grouped-query heads read their K / V head's planes (h * Hkv / H);
//     key splits (attn_split.h) when the grid leaves CU slots idle;
//     slice-sized persistent grids under a CU budget (nos::xcd_chunk).
//
// nos_attn_h3g_lse also stores every query row's log-sum-exp (natural log of
// sum_j exp(scale q_i . k_j) over the keys the row sees) for the backward
// (attention_h3g_bwd.hip); O is the same bits with or without it.
//
// nos_attn_h3g_cache / nos_attn_h3g_cache_ring run the same kernel over the
// K / V caches of a decoder tenant for a step of several tokens (an extend
// chunk, a long windowed prefill): the query positions come from device-side
// counters, the pre-pass and the tile loop are bounded by them (template
// parameter CACHE; attn_kv_planes.h 1', 3').
#include <float.h>
#include <limits.h>
#include <math.h>

#include "attn_kv_planes.h"
#include "attn_split.h"
#include "common.h"
#include "lds_pipe.h"
#include "split_f16.h"

namespace {

constexpr int IMG = KVB * 64 * 2;       // one 64-dim fp16 piece image: 32 rows x 128 B = 4 KiB
constexpr float RESCALE_THR = 8.f;      // log2 units
constexpr int HW = 8;                   // waves per workgroup
constexpr int QB = 32 * HW;             // query rows per workgroup

__device__ __forceinline__ int kswz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int vswz(int row) { return ((row >> 1) & 1) << 2; }

using nos::dma_wait_publish;
using nos::glds16;  // the asm form: in-flight tiles are not drained before every LDS read
using nos::glds16_s;

// ---------------------------------------------------------------- 4. attention
// CACHE: the keys are a K / V cache of Skv rows (slots) per sequence, attended by a step of Sq tokens at
// the device-side counters cs.pos (nos_attn_h3g_cache*): every item derives its sequence's key count,
// mask offset and tile range from pos[b], so one launch shape serves every step.  PLAIN: query i sees the
// keys 0 .. min(pos[b] + i, Skv - 1) -- the causal mask with a per-sequence off (CAUSAL is set).  RING:
// the slots of a sliding window's ring in slot order, masked per element (kv_ring.h; CAUSAL is clear).
enum { NO_CACHE = 0, PLAIN_CACHE = 1, RING_CACHE = 2 };

template <int D, bool CAUSAL, bool ROPE, bool PERSIST, int CACHE = NO_CACHE>
__global__ __launch_bounds__(64 * HW, D == 64 ? 2 : 1) void attn_h3g_kernel(
    const float* __restrict__ q, int ldq, long long bsq, const _Float16* __restrict__ kvs,
    const float* __restrict__ kvsc, float* __restrict__ o, int ldo, long long bso, int B, int H, int Hkv, int Sq,
    int Skv, float c, int nqb, int nsplit, float* __restrict__ part, const float* __restrict__ rc,
    const float* __restrict__ rs, float* __restrict__ lse, CacheStep cs) {
  constexpr int NH = D / 64;                 // 64-dim halves
  constexpr int NKS = D / 16;                // 16-deep MFMA steps over D
  constexpr int STAGE = 4 * NH * IMG;
  constexpr int PPW = 16 * NH / HW;          // 1 KiB DMA pieces per wave per tile
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int nwg = B * H * nqb * nsplit;
  nos::XcdChunk chunk;
  if constexpr (PERSIST) {
    chunk = nos::xcd_chunk(blockIdx.x, gridDim.x, nwg);
  } else {
    chunk.first = nos::xcd_remap(blockIdx.x, nwg);
    chunk.end = chunk.first + 1;
    chunk.step = 1;
  }
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int r = lane & 31;
  const int hh = lane >> 5;

  int koff[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) koff[ks] = r * 128 + (((2 * ks + hh) ^ kswz(r)) << 4);
  const int g16 = (lane >> 4) & 1;
  const int tq = (lane & 15) >> 2;
  const int tp = lane & 3;
  const int vlb = (tq >> 1) & 1;
  int voff[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
    voff[db] = (4 * hh + tq) * 128 + (((4 * (db ^ vlb)) + 2 * g16 + (tp >> 1)) << 4) + 8 * (tp & 1);

  const int skvp = padded_keys(Skv);
  int skv = Skv, ntiles = skvp / KVB;  // the keys an item attends (CACHE: its sequence's, set per item)
  int off = Skv - Sq;  // query i sees keys <= i + off (causal; 0 for self-attention; CACHE: pos[b])
  int soff[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = wid * PPW + i;
    const int img = p >> 2, plane = img / NH, half = img % NH;
    const int row = (p & 3) * 8 + (lane >> 3);
    const int lc = (lane & 7) ^ (plane < 2 ? kswz(row) : vswz(row));
    soff[i] = (row * 4 + plane) * D + half * 64 + lc * 8;
  }

  for (int w = chunk.first; w < chunk.end; w += chunk.step) {
    if (PERSIST && w != chunk.first) __syncthreads();
    const int sp = w % nsplit;
    const int wq = w / nsplit;
    const int b = wq / (H * nqb);
    const int rem = wq - b * (H * nqb);
    const int h = rem / nqb;
    const int qb = CAUSAL ? nqb - 1 - (rem - h * nqb) : rem - h * nqb;  // causal: the longest rows first
    const int hk = h / (H / Hkv);
    const int q0 = qb * QB;
    int pmax = 0, pmod = 0, plo = 0, phi = -1;  // RING: the step's last position and its slot; the positions this block sees
    bool counted = true;                        // RING: the counter lies in [0, limit) (else: zero rows)
    int rpos = 0;                               // CACHE: the counter as the rotary tables are read at (any value)
    if constexpr (CACHE != NO_CACHE) rpos = max(-(1 << 30), min(cs.pos[b], 1 << 30));
    if constexpr (CACHE == PLAIN_CACHE) {
      off = max(min(rpos, Skv), -Sq);  // a counter past the cache sees all of it, one before it nothing
      skv = min(off + Sq, Skv);
      ntiles = padded_keys(skv) / KVB;
    }
    if constexpr (CACHE == RING_CACHE) {
      off = rpos;
      counted = off >= 0 && off < cs.limit;
      if (!counted) off = 0;
      pmax = off + Sq - 1;
      pmod = nos::ring_mod(pmax, Skv);
      plo = nos::ring_oldest(off + q0, pmax, Skv, cs.W);
      phi = off + min(q0 + QB, Sq) - 1;
    }
    int nt_item = CAUSAL ? min(ntiles, (min(q0 + QB, Sq) - 1 + off) / KVB + 1) : ntiles;
    if constexpr (CACHE != NO_CACHE) nt_item = counted ? max(nt_item, 0) : 0;  // rows before position 0 see no tile
    const int tps = (nt_item + nsplit - 1) / nsplit;
    const int t0 = sp * tps, t1 = min(nt_item, t0 + tps);
    const float ksc = kvsc[(b * Hkv + hk) * 2], vinv = 1.f / kvsc[(b * Hkv + hk) * 2 + 1];

    // ---- Q pieces: lane holds Q[row][16 ks + 8 hh .. +7] * c * 2^e (rotated first)
    const int qrow = q0 + wid * 32 + r;
    const int qr = min(qrow, Sq - 1);
    f16x8_t qf[NKS][2];
    float fs;
    {
      const float* qp = q + b * bsq + (long long)qr * ldq + h * D + 8 * hh;
      float x[NKS][8];
      float mx = 0.f;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const float4 x0 = *reinterpret_cast<const float4*>(qp + 16 * ks);
        const float4 x1 = *reinterpret_cast<const float4*>(qp + 16 * ks + 4);
        x[ks][0] = x0.x; x[ks][1] = x0.y; x[ks][2] = x0.z; x[ks][3] = x0.w;
        x[ks][4] = x1.x; x[ks][5] = x1.y; x[ks][6] = x1.z; x[ks][7] = x1.w;
      }
      if constexpr (ROPE) {  // partner dims d +- D/2 are ks +- NKS/2 of this same lane
        // the table row of the query's position (CACHE: clamped to the tables, as rotary_at does)
        const int rr = CACHE != NO_CACHE ? max(0, min(qr + rpos, cs.R - 1)) : qr + off;
        const float* cr = rc + (long long)rr * D + 8 * hh;
        const float* sr = rs + (long long)rr * D + 8 * hh;
        float y[NKS][8];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float cv = cr[16 * ks + j], sv = sr[16 * ks + j];
            y[ks][j] = ks < NKS / 2 ? fmaf(x[ks][j], cv, -x[ks + NKS / 2][j] * sv)
                                    : fmaf(x[ks][j], cv, x[ks - NKS / 2][j] * sv);
          }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
          for (int j = 0; j < 8; ++j) x[ks][j] = y[ks][j];
      }
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(x[ks][j]));
      const int e = nos::h3_scale_exp(xor32_max(mx) * c);
      const float qm = c * nos::pow2i(e);
      fs = nos::pow2i(-e) / ksc;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) nos::split8h(x[ks], qm, qf[ks][0], qf[ks][1]);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int p = 0; p < 2; ++p) asm volatile("" : "+v"(qf[ks][p]));
    }

    const _Float16* pb = kvs + (long long)(b * Hkv + hk) * skvp * 4 * D;
    auto stage_piece = [&](int t, int buf, int i) {
      const int p = wid * PPW + i;
      long long o2 = (long long)t * (KVB * 4) * D + soff[i];
      if ((t + 1) * KVB > skv) {  // tail tile: rows past skv re-read the last key (masked)
        const int over = t * KVB + (p & 3) * 8 + (lane >> 3) - (skv - 1);
        if (over > 0) o2 -= (long long)over * 4 * D;
      }
      glds16(pb + o2, smem + buf * STAGE + (p >> 2) * IMG + (p & 3) * 8 * 128);
    };
    auto stage_full = [&](int t, int buf, int i) {  // full tiles: uniform base + per-lane byte offset
      const int p = wid * PPW + i;
      glds16_s(pb + (long long)t * (KVB * 4) * D, (unsigned)soff[i] * 2u,
               smem + buf * STAGE + (p >> 2) * IMG + (p & 3) * 8 * 128);
    };

    f32x16_t oacc[2 * NH];
#pragma unroll
    for (int db = 0; db < 2 * NH; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;
    float m = 0.f, l = 0.f;

    // RING: the next tile from t on with a slot some row of this block sees (block-uniform); else t
    auto next_tile = [&](int t) {
      if constexpr (CACHE == RING_CACHE)
        while (t < t1 && nos::ring_split_rows(t * KVB, min(KVB, skv - t * KVB), plo, phi, skv) == 0) ++t;
      return t;
    };
    const int tf = next_tile(t0);  // the first tile of this item
    if (tf < t1) {
#pragma unroll
      for (int i = 0; i < PPW; ++i) stage_piece(tf, 0, i);
      dma_wait_publish();
    }
    const int qw0 = q0 + wid * 32;  // this wave's first query row (wave-uniform mask test)
    int nth = 0;                    // RING: tiles done (the stage ring's phase when tiles are skipped)
    for (int t = tf, tn; t < t1; t = tn) {
      const int buf = CACHE == RING_CACHE ? (nth++ & 1) : (t - t0) & 1;
      tn = next_tile(t + 1);
      if (tn < t1) {
        if ((tn + 1) * KVB <= skv) {
#pragma unroll
          for (int i = 0; i < PPW; ++i) stage_full(tn, buf ^ 1, i);
        } else {
#pragma unroll
          for (int i = 0; i < PPW; ++i) stage_piece(tn, buf ^ 1, i);
        }
      }
      const unsigned char* st = smem + buf * STAGE;

      f32x16_t s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          f16x8_t a[2];
#pragma unroll
          for (int pc = 0; pc < 2; ++pc)
            a[pc] = *reinterpret_cast<const f16x8_t*>(st + (pc * NH + hf) * IMG + koff[ks]);
          s = nos::mma3h(a, qf[hf * 4 + ks], s);
        }
      if ((t + 1) * KVB > skv) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (t * KVB + (i & 3) + 8 * (i >> 2) + 4 * hh >= skv) s[i] = -INFINITY;
      }
      if constexpr (CACHE == RING_CACHE) {  // the window, per element: the slots hold positions in no order
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (!nos::ring_visible_m(t * KVB + (i & 3) + 8 * (i >> 2) + 4 * hh, qrow + off, pmax, pmod, skv, cs.W))
            s[i] = -INFINITY;
      }
      if (CAUSAL && t * KVB + KVB - 1 > qw0 + off) {  // a diagonal tile of this wave
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (t * KVB + (i & 3) + 8 * (i >> 2) + 4 * hh > qrow + off) s[i] = -INFINITY;
      }
      float mt = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mt = fmaxf(mt, s[i]);
      // a fully masked row (causal; a split of early keys) keeps a finite
      // reference -1e30; the new reference is set directly (m + delta would
      // lose a real maximum against 1e30 and break P <= 2^8)
      const float mnew = fmaxf(xor32_max(mt) * fs, -1e30f);
      if (t == tf) {
        m = mnew;
      } else if (!__all(mnew - m <= RESCALE_THR)) {
        const float mref = fmaxf(mnew, m);
        const float alpha = __builtin_amdgcn_exp2f(m - mref);
        m = mref;
        l *= alpha;
#pragma unroll
        for (int db = 0; db < 2 * NH; ++db)
#pragma unroll
          for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
      }
      // packed: score -> exp2 units as v_pk_fma_f32 on key pairs, the row sum as
      // v_pk_add_f32 into two pair accumulators -- the same four partial sums in
      // the same order as four scalar ones (bit-identical), half the instructions
      f16x8_t pf[2][2];
      f32x2_t ls2[2] = {f32x2_t{0.f, 0.f}, f32x2_t{0.f, 0.f}};
      const f32x2_t fs2 = {fs, fs}, nm2 = {-m, -m};
#pragma unroll
      for (int j2 = 0; j2 < 8; ++j2) {
        const f32x2_t e2 = __builtin_elementwise_fma(f32x2_t{s[2 * j2], s[2 * j2 + 1]}, fs2, nm2);
        const f32x2_t x = {__builtin_amdgcn_exp2f(e2.x), __builtin_amdgcn_exp2f(e2.y)};
        ls2[j2 & 1] += x;
        nos::set_pair(pf, j2, x);
      }
      l += (ls2[0].x + ls2[0].y) + (ls2[1].x + ls2[1].y);
#pragma unroll
      for (int db = 0; db < 2 * NH; ++db)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          f16x8_t a[2];
#pragma unroll
          for (int pc = 0; pc < 2; ++pc) {
            const unsigned char* base = st + ((2 + pc) * NH + (db >> 1)) * IMG + voff[db & 1] + s2 * 16 * 128;
            const s16x4_t lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, base));
            const s16x4_t hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4_t, base + 8 * 128));
            const s16x8_t a16 = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
            a[pc] = __builtin_bit_cast(f16x8_t, a16);
          }
          oacc[db] = nos::mma3h(a, pf[s2], oacc[db]);
        }
      dma_wait_publish();
    }

    const float lt = xor32_sum(l);
    const int ldh = H * D;
    if (nsplit > 1) {  // unnormalised partial (O on the unit scale, m, l) of this key range
      if (qrow < Sq) {
        const long long row = part_row(sp, B, b, Sq, qrow);
        float* op = part_o(part, row, ldh, D, h);
#pragma unroll
        for (int db = 0; db < 2 * NH; ++db) nos::store_acc32(op + 32 * db, oacc[db], vinv, hh);
        if (hh == 0) {
          float* ml = part_ml(part, nsplit, B, Sq, H, ldh, row, h);
          ml[0] = tf < t1 ? m : -1e30f;
          ml[1] = lt;
        }
      }
      continue;
    }
    // CACHE: a row that sees no key (a bad counter, a position before 0) ends as zeros
    const float inv = CACHE != NO_CACHE && !(lt > 0.f) ? 0.f : vinv / lt;
    if (qrow < Sq) {
      float* op = o + b * bso + (long long)qrow * ldo + h * D;
#pragma unroll
      for (int db = 0; db < 2 * NH; ++db) nos::store_acc32(op + 32 * db, oacc[db], inv, hh);
      // m: the reference in log2 units, lt: the row sum against it; (m + log2 lt) ln 2 with one
      // rounding at the row's magnitude (a backward recomputes P = exp(s - lse) from it)
      if (lse != nullptr && hh == 0)
        lse[((long long)b * H + h) * Sq + qrow] =
            fmaf(m, 0.6931471805599453f, __builtin_amdgcn_logf(lt) * 0.6931471805599453f);
    }
  }  // items
}

struct Layout {
  long long planes, absmax, scales, part, total;
  int skvp;
};

Layout layout(int B, int H, int Hkv, int Sq, int Skv, int D) {
  Layout L;
  L.skvp = padded_keys(Skv);
  L.planes = 0;
  L.absmax = align256((long long)B * Hkv * L.skvp * 4 * D * 2);
  L.scales = L.absmax + align256((long long)B * Hkv * abs_chunks(Skv) * 2 * 4);
  L.part = L.scales + align256((long long)B * Hkv * 2 * 4);
  L.total = L.part + part_bytes(B, H, Sq, D);
  return L;
}

int g_kvsplit = 0;  // 0: auto

}  // namespace

// Workspace bytes of nos_attn_h3g (K / V planes, scales, key-split partials).
NOS_API long long nos_attn_h3g_workspace(int B, int H, int Hkv, int Sq, int Skv, int D) {
  if (!attn_dims_ok(B, H, Hkv, Sq, Skv, D)) return -1;
  return layout(B, H, Hkv, Sq, Skv, D).total;
}

NOS_API int nos_attn_h3g_set_kvsplit(int n) {
  if (n < 0 || n > MAX_SPLIT) return (int)hipErrorInvalidValue;
  g_kvsplit = n;
  return 0;
}

namespace {

// the attention launch of every entry point: the kernel's instantiation for (D, causal, rope, CACHE),
// persistent under a CU budget; a plain cache is causal, a ring is masked per element instead
template <int D, bool CZ, int CACHE, class... A>
int launch_h3g_d(bool rope, long long items, hipStream_t stream, A... args) {
  constexpr size_t lds = 2 * 4 * (D / 64) * IMG;
  if (rope)
    return nos::launch_items(attn_h3g_kernel<D, CZ, true, true, CACHE>, attn_h3g_kernel<D, CZ, true, false, CACHE>,
                             64 * HW, lds, items, stream, args...);
  return nos::launch_items(attn_h3g_kernel<D, CZ, false, true, CACHE>, attn_h3g_kernel<D, CZ, false, false, CACHE>,
                           64 * HW, lds, items, stream, args...);
}
template <int CACHE, class... A>
int launch_h3g(int D, bool causal, bool rope, long long items, hipStream_t stream, A... args) {
  if constexpr (CACHE != RING_CACHE) {
    if (causal || CACHE == PLAIN_CACHE)
      return D == 64 ? launch_h3g_d<64, true, CACHE>(rope, items, stream, args...)
                     : launch_h3g_d<128, true, CACHE>(rope, items, stream, args...);
  }
  if constexpr (CACHE != PLAIN_CACHE)
    return D == 64 ? launch_h3g_d<64, false, CACHE>(rope, items, stream, args...)
                   : launch_h3g_d<128, false, CACHE>(rope, items, stream, args...);
  return (int)hipErrorInvalidValue;
}

// the one host path of nos_attn_h3g (lse == nullptr) and nos_attn_h3g_lse
int attn_h3g_run(const float* q, int ldq, long long bsq, const Rows& k, const Rows& v, float* o, int ldo, long long bso,
                 int B, int H, int Hkv, int Sq, int Skv, int D, int causal, float scale, const float* rope_cos,
                 const float* rope_sin, float rope_bound, void* ws, long long ws_bytes, float* lse,
                 hipStream_t stream) {
  if (!attn_call_ok(B, H, Hkv, Sq, Skv, D, causal, scale, ws, ws_bytes, nos_attn_h3g_workspace) ||
      !Rows{q, ldq, bsq}.ok(H, D) || !Rows{o, ldo, bso}.ok(H, D) || !k.ok(Hkv, D) || !v.ok(Hkv, D))
    return (int)hipErrorInvalidValue;
  if ((rope_cos == nullptr) != (rope_sin == nullptr) || (rope_cos && !(rope_bound > 0.f)))
    return (int)hipErrorInvalidValue;
  // query row i is rotated at table row i + Skv - Sq: with more queries than keys the first rows have none
  if (rope_cos && Sq > Skv) return (int)hipErrorInvalidValue;
  const Layout L = layout(B, H, Hkv, Sq, Skv, D);
  if ((long long)B * H * ((Sq + QB - 1) / QB) * MAX_SPLIT > (1LL << 30) || (long long)B * Hkv * L.skvp * 4 * D > INT_MAX * 8LL)
    return (int)hipErrorInvalidValue;
  auto* base = static_cast<unsigned char*>(ws);
  auto* kvs = reinterpret_cast<_Float16*>(base + L.planes);
  auto* absmax = reinterpret_cast<float*>(base + L.absmax);
  auto* kvsc = reinterpret_cast<float*>(base + L.scales);
  auto* part = reinterpret_cast<float*>(base + L.part);
  launch_kv_prepass(k, v, absmax, kvsc, kvs, B, Hkv, Skv, D, rope_cos ? rope_bound : 1.f, rope_cos, rope_sin, stream);
  if (int rc = (int)hipGetLastError()) return rc;
  const float c = scale * nos::LOG2E;
  const int nqb = (Sq + QB - 1) / QB;
  const long long nwg1 = (long long)B * H * nqb;
  const int nsplit = pick_split(g_kvsplit, nwg1, L.skvp / KVB, D == 64 ? 2 : 1);
  const int rc = launch_h3g<NO_CACHE>(D, causal != 0, rope_cos != nullptr, nwg1 * nsplit, stream, q, ldq, bsq, kvs, kvsc,
                                      o, ldo, bso, B, H, Hkv, Sq, Skv, c, nqb, nsplit, part, rope_cos, rope_sin, lse,
                                      CacheStep{});
  if (rc != 0 || nsplit == 1) return rc;
  if (lse != nullptr) return run_merge<0, false, true>(part, o, B, H, D, Sq, nsplit, ldo, bso, stream, lse);
  return run_merge<0, false, false>(part, o, B, H, D, Sq, nsplit, ldo, bso, stream);
}
}  // namespace

// O = softmax(scale Q K^T [causal]) V for fp32 q [B, Sq, H, D], k / v
// [B, Skv, Hkv, D] (token row strides ld*, batch strides bs*, each head's D
// dims contiguous; H % Hkv == 0: grouped-query heads) into o [B, Sq, H, D]
// (ldo, bso).  D = 64 or 128.  causal: query i attends keys <= i + Skv - Sq.
// rope_cos / rope_sin (fp32 [Skv][D], or null): rotate Q (rows i + Skv - Sq)
// and K (rows = key positions) by rotate_half first; rope_bound >=
// max |cos| + max |sin| of the tables (bounds the rotated keys); refused
// with Sq > Skv, causal or not (no table row for the first queries).  ws: at
// least nos_attn_h3g_workspace() bytes, 256-byte aligned.
NOS_API int nos_attn_h3g(const float* q, int ldq, long long bsq, const float* k, int ldk, long long bsk,
                         const float* v, int ldv, long long bsv, float* o, int ldo, long long bso, int B, int H, int Hkv,
                         int Sq, int Skv, int D, int causal, float scale, const float* rope_cos, const float* rope_sin,
                         float rope_bound, void* ws, long long ws_bytes, hipStream_t stream) {
  return attn_h3g_run(q, ldq, bsq, {k, ldk, bsk}, {v, ldv, bsv}, o, ldo, bso, B, H, Hkv, Sq, Skv, D, causal, scale,
                      rope_cos, rope_sin, rope_bound, ws, ws_bytes, nullptr, stream);
}

// nos_attn_h3g that also writes lse [B][H][Sq] (contiguous fp32): the natural
// log of sum_j exp(scale q_i . k_j) over the keys query row i sees.
NOS_API int nos_attn_h3g_lse(const float* q, int ldq, long long bsq, const float* k, int ldk, long long bsk,
                             const float* v, int ldv, long long bsv, float* o, int ldo, long long bso, int B, int H,
                             int Hkv, int Sq, int Skv, int D, int causal, float scale, const float* rope_cos,
                             const float* rope_sin, float rope_bound, void* ws, long long ws_bytes, float* lse,
                             hipStream_t stream) {
  if (lse == nullptr || ((uintptr_t)lse & 3)) return (int)hipErrorInvalidValue;
  return attn_h3g_run(q, ldq, bsq, {k, ldk, bsk}, {v, ldv, bsv}, o, ldo, bso, B, H, Hkv, Sq, Skv, D, causal, scale,
                      rope_cos, rope_sin, rope_bound, ws, ws_bytes, lse, stream);
}

// ---------------------------------------------------------------- over K / V caches
// Workspace bytes of nos_attn_h3g_cache / nos_attn_h3g_cache_ring over caches of L rows (slots): sized
// from L alone, whatever the counters hold.
NOS_API long long nos_attn_h3g_cache_workspace(int B, int H, int Hkv, int Sq, int L, int D) {
  return nos_attn_h3g_workspace(B, H, Hkv, Sq, L, D);
}

namespace {

// the one host path of nos_attn_h3g_cache (window == 0) and nos_attn_h3g_cache_ring: nothing here reads
// pos -- the grid, the split count and the workspace layout follow L, so a captured graph serves every step
int attn_h3g_cache_run(const float* q, int ldq, long long bsq, const float* kc, const float* vc, const int* pos,
                       const float* rope_cos, const float* rope_sin, int R, float* o, int ldo, long long bso, int B,
                       int H, int Hkv, int Sq, int L, int D, float scale, void* ws, long long ws_bytes, int window,
                       int limit, hipStream_t stream) {
  if (!attn_call_ok(B, H, Hkv, Sq, L, D, 0, scale, ws, ws_bytes, nos_attn_h3g_cache_workspace) ||
      !Rows{q, ldq, bsq}.ok(H, D) || !Rows{o, ldo, bso}.ok(H, D) || !Rows{kc, Hkv * D, 0}.ok(Hkv, D) ||
      !Rows{vc, Hkv * D, 0}.ok(Hkv, D) || pos == nullptr || ((uintptr_t)pos & 3))
    return (int)hipErrorInvalidValue;
  if ((rope_cos == nullptr) != (rope_sin == nullptr) || (rope_cos && R <= 0)) return (int)hipErrorInvalidValue;
  if (window != 0 && !nos::ring_args_ok(L, Sq, window, limit, rope_cos != nullptr, R)) return (int)hipErrorInvalidValue;
  const Layout lay = layout(B, H, Hkv, Sq, L, D);
  if ((long long)B * H * ((Sq + QB - 1) / QB) * MAX_SPLIT > (1LL << 30) || (long long)B * Hkv * lay.skvp * 4 * D > INT_MAX * 8LL ||
      L > (1 << 30) - Sq)
    return (int)hipErrorInvalidValue;
  auto* base = static_cast<unsigned char*>(ws);
  auto* kvs = reinterpret_cast<_Float16*>(base + lay.planes);
  auto* absmax = reinterpret_cast<float*>(base + lay.absmax);
  auto* kvsc = reinterpret_cast<float*>(base + lay.scales);
  auto* part = reinterpret_cast<float*>(base + lay.part);
  const CacheStep cs{pos, Sq, window, limit, R};
  launch_kv_cache_prepass(kc, vc, absmax, kvsc, kvs, B, Hkv, L, D, cs, stream);
  if (int rc = (int)hipGetLastError()) return rc;
  const float c = scale * nos::LOG2E;
  const int nqb = (Sq + QB - 1) / QB;
  const long long nwg1 = (long long)B * H * nqb;
  const int nsplit = pick_split(g_kvsplit, nwg1, lay.skvp / KVB, D == 64 ? 2 : 1);
  const bool rope = rope_cos != nullptr;
  float* no_lse = nullptr;
  const int rc = window == 0
                     ? launch_h3g<PLAIN_CACHE>(D, true, rope, nwg1 * nsplit, stream, q, ldq, bsq, kvs, kvsc, o, ldo, bso,
                                               B, H, Hkv, Sq, L, c, nqb, nsplit, part, rope_cos, rope_sin, no_lse, cs)
                     : launch_h3g<RING_CACHE>(D, false, rope, nwg1 * nsplit, stream, q, ldq, bsq, kvs, kvsc, o, ldo, bso,
                                              B, H, Hkv, Sq, L, c, nqb, nsplit, part, rope_cos, rope_sin, no_lse, cs);
  if (rc != 0 || nsplit == 1) return rc;
  return run_merge<0, false, false>(part, o, B, H, D, Sq, nsplit, ldo, bso, stream);
}
}  // namespace

// The h3 flash attention of a step of Sq tokens over K / V caches: q fp32 [B, Sq, H, D] (ldq, bsq as in
// nos_attn_h3g), kc / vc fp32 [B, L, Hkv, D] contiguous and 16-byte aligned (the keys as stored: already
// rotated), pos i32 [B] on the device.  Query i of sequence b, at position pos[b] + i, attends the keys
// 0 .. min(pos[b] + i, L - 1); rows at and past pos[b] + Sq are never read (the pre-pass and the kernel are
// bounded by the counter), so a step's work follows pos, not L.  rope_cos / rope_sin (fp32 [R][D], or
// null): Q alone is rotated, at table row pos[b] + i clamped to the tables.  A row that sees no key is
// zeros.  ws: at least nos_attn_h3g_cache_workspace() bytes, 256-byte aligned.  Nothing on the host reads
// pos: one captured graph serves every step.
NOS_API int nos_attn_h3g_cache(const float* q, int ldq, long long bsq, const float* kc, const float* vc, const int* pos,
                               const float* rope_cos, const float* rope_sin, int R, float* o, int ldo, long long bso,
                               int B, int H, int Hkv, int Sq, int L, int D, float scale, void* ws, long long ws_bytes,
                               hipStream_t stream) {
  return attn_h3g_cache_run(q, ldq, bsq, kc, vc, pos, rope_cos, rope_sin, R, o, ldo, bso, B, H, Hkv, Sq, L, D, scale,
                            ws, ws_bytes, 0, 0, stream);
}

// nos_attn_h3g_cache over ring caches [B, C, Hkv, D] (kv_ring.h) with a sliding window: the query at
// position p attends the positions max(0, p - window + 1) .. p, position j in slot j % C, after the
// step's rows were written.  Only the slots some row of the step sees are read (the others, stale or
// never written, get zero planes); a counter outside [0, limit) gives zero rows.  window < Sq is legal (a
// long windowed prefill).  Arguments checked as nos_attn_decode_ring's: min(limit, window + Sq - 1) <= C <=
// limit, Sq <= C, limit <= R with rotary tables.
NOS_API int nos_attn_h3g_cache_ring(const float* q, int ldq, long long bsq, const float* kc, const float* vc,
                                    const int* pos, const float* rope_cos, const float* rope_sin, int R, float* o,
                                    int ldo, long long bso, int B, int H, int Hkv, int Sq, int C, int D, float scale,
                                    void* ws, long long ws_bytes, int window, int limit, hipStream_t stream) {
  if (window < 1) return (int)hipErrorInvalidValue;
  return attn_h3g_cache_run(q, ldq, bsq, kc, vc, pos, rope_cos, rope_sin, R, o, ldo, bso, B, H, Hkv, Sq, C, D, scale,
                            ws, ws_bytes, window, limit, stream);
}
