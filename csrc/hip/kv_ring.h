// Ring K / V caches of a sliding-window decoder (decode.hip): the slot and visibility arithmetic,
// shared by the kernels and (through the nos_ring_* wrappers) by the CPU tests.
//
// A ring cache has C slots; position p lives in slot p % C.  A query at position qpos attends the
// W positions max(0, qpos - W + 1) .. qpos.  A step of S tokens writes its rows first and then
// attends, which is correct when C >= W + S - 1: the row a fresh row replaces is at a position
// <= qpos - W for every query of the step.  All arithmetic is int: the callers keep positions below
// 2^30 (the host checks limit, the kernels drop a counter outside [0, limit)).
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

namespace nos {

// a mod C in [0, C) for any a (% of a negative int is negative)
__host__ __device__ inline int ring_mod(int a, int C) {
  const int m = a % C;
  return m < 0 ? m + C : m;
}

// the slot of position p; -1 for a position that is not stored (p < 0 or p >= limit): no address is
// formed from it
__host__ __device__ inline int ring_slot(int p, int C, int limit) { return (p < 0 || p >= limit) ? -1 : p % C; }

// the position slot s (0 <= s < C) holds once the step ending at position pmax has written its rows:
// pmax - ((pmax - s) mod C), the largest position <= pmax of that slot; negative: never written
__host__ __device__ inline int ring_position(int s, int pmax, int C) {
  const int m = ring_mod(pmax, C);  // the slot of pmax
  return s <= m ? pmax - m + s : pmax - m + s - C;
}

// the query at qpos (of the step ending at pmax) sees slot s
__host__ __device__ inline bool ring_visible(int s, int qpos, int pmax, int C, int W) {
  const int a = ring_position(s, pmax, C);
  return a >= 0 && a <= qpos && a > qpos - W;
}

// ring_visible with m = ring_mod(pmax, C) computed once by the caller (a kernel's inner loop)
__host__ __device__ inline bool ring_visible_m(int s, int qpos, int pmax, int m, int C, int W) {
  const int a = s <= m ? pmax - m + s : pmax - m + s - C;
  return a >= 0 && a <= qpos && a > qpos - W;
}

// the checks of every entry point that takes a ring cache of C slots at a step of S rows: window W,
// positions below limit (<= the R rows of the rotary tables, when there are any)
inline bool ring_args_ok(int C, int S, int W, int limit, bool rope, int R) {
  if (W < 1 || limit < 1 || limit > (1 << 30) || C > limit || S > C) return false;
  const long long need = (long long)W + S - 1;
  if (C < (need < limit ? need : limit)) return false;
  return !rope || limit <= R;
}

// the positions some query row of a launch sees: rows at qlo .. qhi (<= pmax) see lo .. qhi, lo the
// oldest position the first row's window and the ring still hold; lo > qhi: none
__host__ __device__ inline int ring_oldest(int qlo, int pmax, int C, int W) {
  const int w = qlo - W + 1, r = pmax - C + 1;
  const int lo = w > r ? w : r;
  return lo > 0 ? lo : 0;
}

// how many leading slots of the split k0 .. k0 + n - 1 reach its last slot holding a position in
// lo .. hi (0 <= lo, hi - lo < C); 0: the split holds none of them
__host__ __device__ inline int ring_split_rows(int k0, int n, int lo, int hi, int C) {
  if (hi < lo || n <= 0) return 0;
  const int sl = lo % C, sh = hi % C, last = k0 + n - 1;
  if (sl > sh && last >= sl) return n;  // the range wraps and its upper piece sl .. C - 1 reaches the split's end
  if ((sl > sh || last >= sl) && k0 <= sh) return (sh < last ? sh : last) - k0 + 1;
  return 0;
}

}  // namespace nos
