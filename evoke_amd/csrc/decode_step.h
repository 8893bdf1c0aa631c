// decode_step.h -- device helpers shared by the four per-token bookkeeping kernels (beam.hip, sample.hip, hf_beam.hip, hf_sample.hip):
// the (value, lowest index) order and its block reductions, the batched row walk, the per-thread candidate list and its block rounds,
// the row rewrite in the winners' order, the sorted list of finished hypotheses, Hugging Face's logits processors, the inverse-CDF draw
// and the position advance.  Device code only: every kernel, entry point and LDS layout stays in its own file.  NT = threads per workgroup.
#pragma once
#include "common.h"

namespace {

constexpr int NO_CAND = 0x7fffffff;   // index of "no comparable candidate": loses every tie
constexpr int NGRAM_MAX = 8;          // largest no_repeat_ngram_size the entry points accept

// ---- the total order of the candidates: larger value, then LOWEST index (torch.sort(descending=True)'s order on distinct scores)
__device__ __forceinline__ bool better(float v, int i, float than_v, int than_i) { return v > than_v || (v == than_v && i < than_i); }
__device__ __forceinline__ void shfl_argmax(float& v, int& i) {           // over the 64 lanes, result in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}
// block-wide reductions: per-wave shuffle, then one LDS round; the result is returned to every thread
template <int NT>
__device__ __forceinline__ void block_argmax(float& v, int& i, float* s_val, int* s_idx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  shfl_argmax(v, i);
  __syncthreads();                    // (the scratch words may still be read from an earlier round)
  if (lane == 0) { s_val[wave] = v; s_idx[wave] = i; }
  __syncthreads();
  v = s_val[0]; i = s_idx[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) if (better(s_val[w], s_idx[w], v, i)) { v = s_val[w]; i = s_idx[w]; }
}
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* s_val) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) s_val[wave] = v;
  __syncthreads();
  v = s_val[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) v += s_val[w];
  return v;
}
// order-preserving image of a float in the unsigned integers
__device__ __forceinline__ uint32_t fkey(float f) { const uint32_t b = __float_as_uint(f); return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }

// ---- a thread's strided share of one row of n floats -> use(column, value).  The share is requested in one batch (UNR loads in flight)
// before the first value is used: the step kernels are latency bound, and one dependent L2 round trip per element (23 per thread at beam 4,
// V = 1444) was most of the beam step's time.
template <int NT, class Use>
__device__ __forceinline__ void walk_row(const float* row, int n, Use&& use) {
  constexpr int UNR = 8;
  for (int w0 = threadIdx.x; w0 < n; w0 += NT * UNR) {
    float lv[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) { const int w = w0 + NT * u; lv[u] = w < n ? row[w] : 0.f; }
#pragma unroll
    for (int u = 0; u < UNR; ++u) { const int w = w0 + NT * u; if (w < n) use(w, lv[u]); }
  }
}

// ---- a thread's sorted list of its best candidates (registers: every index is a compile-time constant).  Which thread sees which
// candidate does not matter: the order is total.
template <int CAP>
struct CandList {
  float v[CAP]; int i[CAP];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < CAP; ++j) { v[j] = -INFINITY; i[j] = NO_CAND; }
  }
  __device__ __forceinline__ void insert(float nv, int ni, int depth) {     // depth <= CAP entries are kept
    if (depth == CAP && !better(nv, ni, v[CAP - 1], i[CAP - 1])) return;    // (cannot enter a full-depth list)
#pragma unroll
    for (int j = 0; j < CAP; ++j)
      if (j < depth && better(nv, ni, v[j], i[j])) { const float tv = v[j]; const int ti = i[j]; v[j] = nv; i[j] = ni; nv = tv; ni = ti; }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < CAP; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[CAP - 1] = -INFINITY; i[CAP - 1] = NO_CAND;
  }
};
// k rounds of a block arg-max over the heads of the threads' lists: round r's winner goes to win_v[r] / win_i[r] (descending), its owner
// pops it.  No comparable candidate left (every remaining value NaN): rank r takes index r * none_stride at -inf, a defined in-range state
// instead of a sentinel that would address rows beyond the study's beams in the caller's rewrite.
template <int NT, int CAP>
__device__ __forceinline__ void pick_rounds(CandList<CAP>& l, int k, int none_stride, float* s_val, int* s_idx, float* win_v, int* win_i) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = 0; r < k; ++r) {
    float best = l.v[0]; int bid = l.i[0];
    shfl_argmax(best, bid);
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bid; }
    __syncthreads();
    if (tid == 0) {
      float fv = s_val[0]; int fi = s_idx[0];
      for (int w = 1; w < NT / 64; ++w) if (better(s_val[w], s_idx[w], fv, fi)) { fv = s_val[w]; fi = s_idx[w]; }
      if (fi == NO_CAND) { fv = -INFINITY; fi = r * none_stride; }
      win_v[r] = fv; win_i[r] = fi;
    }
    __syncthreads();
    if (l.i[0] == win_i[r]) l.pop();    // the owner pops its head
  }
}

// ---- a study's [n][cols] table rewritten IN PLACE from its staged copy in the winners' order (a study's hypotheses only permute among
// themselves): row j <- staged row src_of(j), except column col_new, which takes tok_of(j) (col_new < 0: no such column)
template <int NT, class T, class Src, class Tok>
__device__ __forceinline__ void rewrite_rows(T* g, const T* l, int n, int cols, long col_new, Src&& src_of, Tok&& tok_of) {
  for (int i = threadIdx.x; i < n * cols; i += NT) {
    const int j = i / cols, c = i - j * cols;
    g[i] = c == col_new ? (T)tok_of(j) : l[src_of(j) * cols + c];
  }
}

// ---- the sorted list of a study's n finished hypotheses: score descending, length 0 = empty slot.  An entry enters below every entry that
// is at least as good (Python's stable sort of the appended list), the list is cut to n; f_src remembers where a slot's row comes from:
// an old slot (< n) or the fresh entry f_src - n.  -> whether it entered
__device__ __forceinline__ bool list_insert(double* f_sc, int* f_ln, int* f_src, int n, double s, int len, int fresh) {
  int k = 0;
  while (k < n && f_ln[k] != 0 && !(s > f_sc[k])) ++k;
  if (k >= n) return false;
  for (int q = n - 1; q > k; --q) { f_sc[q] = f_sc[q - 1]; f_ln[q] = f_ln[q - 1]; f_src[q] = f_src[q - 1]; }
  f_sc[k] = s; f_ln[k] = len; f_src[k] = n + fresh;
  return true;
}
// the list's [n][cols] rows follow f_src; fresh_at(e, c) is column c of fresh entry e.  Entries only move DOWN, so walking the slots from
// the bottom up lets a thread read a column before it overwrites it -- no staging
template <int NT, class T, class Fresh>
__device__ __forceinline__ void list_move_rows(T* rows, const int* f_src, int n, int cols, Fresh&& fresh_at) {
  for (int c = threadIdx.x; c < cols; c += NT)
    for (int d = n - 1; d >= 0; --d) {
      const int s = f_src[d];
      if (s != d) rows[(long)d * cols + c] = s < n ? rows[(long)s * cols + c] : (T)fresh_at(s - n, c);
    }
}

// ---- Hugging Face's logits processors on one row x of V entries (global or LDS) from its history h[0 .. cur - 1] (H: the history's
// element type).  An id outside the row touches nothing.  The caller owns the barriers between them: a ban must not be overwritten by a
// penalty's read-modify-write.
// RepetitionPenaltyLogitsProcessor: every distinct id of the history once -- the thread that holds its first occurrence rewrites the entry
template <int NT, class H>
__device__ __forceinline__ void hf_repetition_penalty(float* x, const H* h, int cur, int V, float penalty) {
  for (int c = threadIdx.x; c < cur; c += NT) {
    const H w = h[c];
    bool first = w >= 0 && w < V;
    for (int q = 0; q < c && first; ++q) first = h[q] != w;
    if (first) { const float v = x[w]; x[w] = v < 0.f ? v * penalty : v / penalty; }
  }
}
// NoRepeatNGramLogitsProcessor (0 < g <= cur): every earlier window of g ids that starts like the last g - 1 ids bans its own last id
// (several windows may ban the same id: the same store)
template <int NT, class H>
__device__ __forceinline__ void hf_ban_ngrams(float* x, const H* h, int cur, int V, int g) {
  const int tail = cur - (g - 1);                            // the last g - 1 ids: h[tail .. cur - 1]
  for (int c = threadIdx.x; c + g <= cur; c += NT) {
    bool same = true;
    for (int q = 0; q < g - 1 && same; ++q) same = h[c + q] == h[tail + q];
    const H w = h[c + g - 1];
    if (same && w >= 0 && w < V) x[w] = -INFINITY;
  }
}
// MinLengthLogitsProcessor while cur < min_length (one thread per row; the caller tests, its barrier hangs on the same condition)
__device__ __forceinline__ void hf_min_length(float* x, int eos) { x[eos] = -INFINITY; }

// ---- inverse-CDF draw over the weights w(0 .. V - 1) >= 0 in vocabulary order with the uniform number u: a thread owns a contiguous
// piece, a wave scans its 64 pieces, wave totals meet in LDS.  -> the first column of positive weight whose running sum exceeds u * total;
// the highest column of positive weight when none does (u next to 1: the target >= the rounded total); `none` when no weight is positive.
template <int NT, class W>
__device__ __forceinline__ int draw_inverse_cdf(int V, float u, int none, W&& w, float* s_scan, float* s_val, int* s_idx) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = (V + NT - 1) / NT, c0 = min(V, tid * C), c1 = min(V, c0 + C);
  __syncthreads();                    // what w reads is complete (the caller's threads wrote it); s_scan is free of an earlier draw
  float own = 0.f;
  for (int j = c0; j < c1; ++j) own += w(j);
  float inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
  if (lane == 63) s_scan[wave] = inc;
  __syncthreads();
  float base = 0.f, all = 0.f;
#pragma unroll
  for (int q = 0; q < NT / 64; ++q) { if (q < wave) base += s_scan[q]; all += s_scan[q]; }
  const float target = u * all;
  float run = base + inc - own;
  float cv = -INFINITY; int ci = NO_CAND;                    // the first such column: arg-max of (0, lowest index)
  int last = -1;                                             // the highest column of positive weight
  for (int j = c0; j < c1; ++j) {
    const float k = w(j);
    run += k;
    if (k > 0.f) last = j;
    if (ci == NO_CAND && k > 0.f && run > target) { cv = 0.f; ci = j; }
  }
  block_argmax<NT>(cv, ci, s_val, s_idx);
  if (ci == NO_CAND) {
    float lv = last < 0 ? -INFINITY : 0.f; int li = last < 0 ? NO_CAND : -last;      // highest index = lowest negated index among equal keys
    block_argmax<NT>(lv, li, s_val, s_idx);
    ci = li == NO_CAND ? none : -li;
  }
  return ci;
}

// ---- the LAST workgroup to finish writes *pos_out = pos + 1 (every workgroup has read the position by then); the ticket word counts the
// arrivals and is left at zero for the next launch.  It replaces an add launch per token.
__device__ __forceinline__ void advance_position(long long* pos_out, int* ticket, long pos) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) { *ticket = 0; pos_out[0] = pos + 1; }
  }
}

}  // namespace
