// sample.hip -- one kernel per generated token for everything AttModel._sample does between two decoder steps
// (modules/att_model.py:176-221: the decoding constraint, trigram blocking, the stored log-probability row, the choice of the next word
// -- CaptionModel.sample_next_word, modules/caption_model.py:363-401: greedy arg-max, or temperature + top-k / nucleus filter + a categorical
// draw -- and the finished-row bookkeeping).  The reference walks a per-row Python loop with .item() syncs for the trigrams and a sort +
// scatter + Categorical for the draw; here one workgroup owns one row, the row lives in LDS, and the draw is an inverse CDF over the kept
// entries with a uniform number the caller supplies (no generator state in the kernel: a replayed graph reads a refilled buffer).
// Rows are independent (no hypothesis re-ordering), so unlike beam.hip nothing of the decoder's state is touched.
#include <stdlib.h>
#include "common.h"
#include "decode_step.h"

namespace {

constexpr int NT = 256;            // threads per workgroup (4 waves)
constexpr int V1_MAX = 4096;       // three f32 rows of V1 in LDS

enum { M_GREEDY = 0, M_SAMPLE = 1, M_TOPK = 2, M_TOPP = 3 };

struct SampleP {
  const float* logp; int ld;          // [R][ld] f32 log-probs of the step, V1 valid columns
  int V1, max_len, eos, pad, block_rows, constraint, method;
  float temperature, param;           // param: k of top-k, p of top-p
  const long long* pos;               // device scalar: position being written
  long long* seq;                     // [R][max_len] (in / out)
  unsigned char* unfinished;          // [R] (in / out; written at position 0)
  long long* words;                   // [R] out: tokens fed to the next decoder step
  float* seq_logprobs;                // [R][max_len][V1] or null
  const float* uniforms;              // [R][max_len] or null (greedy)
  long long* pos_out; int* ticket;    // advance: the LAST workgroup to finish writes *pos_out = pos + 1 (every workgroup has read pos by then)
};

__global__ __launch_bounds__(NT) void sample_step_kernel(const SampleP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_val[NT / 64]; __shared__ int s_idx[NT / 64];
  __shared__ float s_scan[NT / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int V1 = p.V1;
  float* x = reinterpret_cast<float*>(smem);                 // [V1] the row after the constraint and the trigram penalty
  int* cnt = reinterpret_cast<int*>(x + V1);                 // [V1] trigram counts; later the row's softmax weights
  float* wgt = reinterpret_cast<float*>(cnt);
  float* kept = wgt + V1;                                    // [V1] weights that survive the filter (stochastic methods only)
  int* l_seq = reinterpret_cast<int*>(p.method == M_GREEDY ? wgt + V1 : kept + V1);      // [max_len]
  const long t = p.pos[0];
  if (t >= 0 && t < p.max_len) {                             // (uniform; a position outside the row writes nothing)
    // ---- 0. everything this workgroup reads, requested in batches: the row, its history, its flags
    const float* row = p.logp + (long)r * p.ld;
    long long* seq = p.seq + (long)r * p.max_len;
    const bool fin = t > 0 && !p.unfinished[r];
    const float u = p.uniforms ? p.uniforms[(long)r * p.max_len + t] : 0.f;
    const bool blocking = t >= 3 && r < p.block_rows;
    for (int c = tid; c < p.max_len; c += NT) l_seq[c] = c < t ? (int)seq[c] : -1;
    walk_row<NT>(row, V1, [&](int w, float v) { x[w] = v; cnt[w] = 0; });
    __syncthreads();
    // ---- 1. decoding constraint: the previous word cannot follow itself
    if (p.constraint && t > 0 && tid == 0) { const int w = l_seq[t - 1]; if (w >= 0 && w < V1) x[w] = -INFINITY; }
    // ---- 2. trigram blocking: every earlier occurrence of (a, b, w) with (a, b) = the last two words counts once against w
    if (blocking) {
      const int a = l_seq[t - 2], b = l_seq[t - 1];
      for (int k = 2 + tid; k <= t - 1; k += NT) {
        const int w = l_seq[k];
        if (l_seq[k - 2] == a && l_seq[k - 1] == b && w >= 0 && w < V1) atomicAdd(&cnt[w], 1);
      }
    }
    __syncthreads();
    // ---- 3. the penalty, the stored row (zeros for a finished row) and the row's arg-max in one pass
    float bv = -INFINITY; int bi = NO_CAND;
    float* out = p.seq_logprobs ? p.seq_logprobs + ((long)r * p.max_len + t) * V1 : nullptr;
    for (int w = tid; w < V1; w += NT) {
      float v = x[w];
      if (blocking) { const int c = cnt[w]; if (c) { v += ((float)c * -0.693f) * 2.0f; x[w] = v; } }
      if (out) out[w] = fin ? 0.f : v;
      if (v > bv) { bv = v; bi = w; }                        // ascending index: ties keep the lowest
    }
    block_argmax<NT>(bv, bi, s_val, s_idx);
    int it = bi == NO_CAND ? 0 : bi;                         // no comparable entry (the whole row NaN / -inf): a defined token, [PAD]'s column
    // ---- 4. the stochastic methods: temperature, filter, inverse-CDF draw
    if (p.method != M_GREEDY && bi != NO_CAND) {
      const float ymax = bv / p.temperature;
      float part = 0.f;
      for (int w = tid; w < V1; w += NT) { const float e = expf(x[w] / p.temperature - ymax); wgt[w] = e; part += e; }
      const float total = block_sum<NT>(part, s_val);        // (its barriers also publish wgt)
      if (p.method == M_SAMPLE) {
        for (int w = tid; w < V1; w += NT) kept[w] = wgt[w];
      } else {
        // The kept set is a prefix of the descending order (ties: lower index first): top-k keeps rank < k, top-p keeps an entry while the
        // cumulative probability BEFORE it is < p.  Both are "F(x_w) < limit" with F(v) = count, or weight, of the entries above v, a step
        // function that only falls as v grows: a bisection over the order-preserving integer image of the floats finds the smallest kept
        // value in <= 32 block reductions (a sort of the padded row would take 66 exchange stages).
        const bool by_count = p.method == M_TOPK;
        const float limit = by_count ? (float)(int)p.param : p.param * total;
        auto above = [&](uint32_t m) {
          float a = 0.f;
          for (int w = tid; w < V1; w += NT) if (fkey(x[w]) > m) a += by_count ? 1.f : wgt[w];
          return block_sum<NT>(a, s_val);
        };
        uint32_t lo = 0x007fffffu, hi = fkey(bv);            // fkey(-inf) .. fkey(row maximum): F(hi) = 0 < limit
        while (lo < hi) {                                    // (uniform: every thread holds the same reduction results)
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (above(mid) < limit) hi = mid; else lo = mid + 1;
        }
        const float front = above(hi);
        float eq = 0.f;
        for (int w = tid; w < V1; w += NT) eq += fkey(x[w]) == hi ? 1.f : 0.f;
        const bool ties = block_sum<NT>(eq, s_val) > 1.f;    // several entries share the boundary value: they enter in index order
        for (int w = tid; w < V1; w += NT) {
          const uint32_t kx = fkey(x[w]);
          bool keep = kx >= hi;
          if (ties && kx == hi) {
            int ahead = 0;
            for (int j = 0; j < w; ++j) ahead += fkey(x[j]) == hi ? 1 : 0;
            keep = front + (float)ahead * (by_count ? 1.f : wgt[w]) < limit;
          }
          kept[w] = keep ? wgt[w] : 0.f;
        }
      }
      it = draw_inverse_cdf<NT>(V1, u, it, [&](int j) { return kept[j]; }, s_scan, s_val, s_idx);
    }
    // ---- 5. finished rows emit [PAD]; a row finishes when it emits [EOS]
    if (tid == 0) {
      bool unf;
      if (t == 0) unf = it != p.eos;
      else {
        unf = !fin;
        if (fin) it = p.pad;
        unf = unf && it != p.eos;
      }
      seq[t] = it;
      p.words[r] = it;
      p.unfinished[r] = unf ? 1 : 0;
    }
  }
  if (p.pos_out) advance_position(p.pos_out, p.ticket, t);
}

}  // namespace

extern "C" {

int evk_sample_step(const float* logp, int32_t ld, int32_t V1, int32_t R, int32_t max_len, const int64_t* pos, int32_t eos, int32_t pad,
                    int32_t block_rows, int32_t decoding_constraint, float temperature, int32_t method, float param, int64_t* seq,
                    unsigned char* unfinished, int64_t* words, float* seq_logprobs, const float* uniforms, int64_t* pos_advance,
                    int32_t* ticket, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EVK_REQUIRE(logp && pos && seq && unfinished && words && R > 0 && V1 > 0 && ld >= V1 && max_len > 0, "sample_step: bad args");
  EVK_REQUIRE(V1 <= V1_MAX, "sample_step: V1 = %d exceeds %d (the row is kept in LDS)", V1, V1_MAX);
  EVK_REQUIRE(method >= M_GREEDY && method <= M_TOPP, "sample_step: method must be 0 (greedy), 1 (sample), 2 (top-k) or 3 (top-p)");
  EVK_REQUIRE(method == M_GREEDY || (uniforms && temperature > 0.f), "sample_step: a stochastic method needs uniforms and temperature > 0");
  EVK_REQUIRE(method != M_TOPK || (param >= 1.f && param <= (float)V1), "sample_step: top-k needs k in [1, V1]");
  EVK_REQUIRE(method != M_TOPP || (param > 0.f && param < 1.f), "sample_step: top-p needs p in (0, 1)");
  EVK_REQUIRE(eos >= 0 && eos < V1 && pad >= 0 && pad < V1 && block_rows >= 0, "sample_step: bad token ids");
  EVK_REQUIRE(!pos_advance || ticket, "sample_step: advancing the position needs a (zero-initialised) ticket word");
  const size_t lds = (size_t)V1 * 4 * (method == M_GREEDY ? 2 : 3) + (size_t)max_len * 4;
  EVK_REQUIRE(lds <= 60000, "sample_step: %zu bytes of row state do not fit LDS", lds);
  SampleP p{logp, ld, V1, max_len, eos, pad, block_rows, decoding_constraint, method, temperature, param,
            reinterpret_cast<const long long*>(pos), reinterpret_cast<long long*>(seq), unfinished, reinterpret_cast<long long*>(words),
            seq_logprobs, uniforms, reinterpret_cast<long long*>(pos_advance), ticket};
  ProfScope ps(EVK_FAM_NORM, s);
  hipLaunchKernelGGL(sample_step_kernel, dim3(R), dim3(NT), lds, s, p);
  return evk_check_launch("sample_step");
}

}  // extern "C"
