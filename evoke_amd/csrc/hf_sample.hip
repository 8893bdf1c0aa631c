// hf_sample.hip -- one kernel per generated token for everything Hugging Face's `generate` does between two decoder steps when it samples or
// decodes greedily (num_beams 1): the standard logits processors in HF's order -- RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
// MinLengthLogitsProcessor, then with do_sample TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper -- the choice of the next token and
// the finished-row bookkeeping.  The distilgpt2 backend's counterpart of sample.hip, which restates the R2Gen reference's own rules
// (log-probability input, trigram penalty, another nucleus definition) and cannot be borrowed: the processors act on the RAW f32 logits (the
// repetition penalty depends on the sign), so this kernel reads the head's output directly and no log_softmax launch precedes it.
// One workgroup owns one row; only the row (and the row's history) lives in LDS, softmax weights are recomputed where they are needed, so a
// vocabulary of 12288 entries fits the 64 KB a workgroup may ask for without a device attribute.  Top-k and top-p both reduce to a VALUE
// threshold -- entries strictly below the k-th largest value leave; an entry stays iff the probability mass of all entries <= its value exceeds
// 1 - p -- found by the bisection over the order-preserving integer image of the floats that sample.hip uses; entries of equal value stay or
// leave together, so no tie ordering exists.  The draw is an inverse CDF over the kept entries in vocabulary order with a uniform number the
// caller supplies (no generator state in the kernel: a replayed graph reads a refilled buffer).
#include <stdlib.h>
#include "common.h"
#include "decode_step.h"

namespace {

constexpr int NT = 256;            // threads per workgroup (4 waves)
constexpr int V_MAX = 12288;       // one f32 row of V in LDS (48 KB)
constexpr int LEN_MAX = 256;       // the row's history in LDS (1 KB)

struct HfSampleP {
  const float* logits; int ld;        // [R][ld] f32 raw logits of the step, V valid columns
  int V, max_len, eos, pad, do_sample, ngram, min_length, top_k;
  float rep_penalty, temperature, top_p;
  const long long* pos;               // device scalar: last filled column of seqs (cur_len = *pos + 1 ids so far, [BOS] included)
  long long* seqs;                    // [R][max_len] (in / out): the new id goes to column cur_len
  unsigned char* unfinished;          // [R] (in / out; the caller sets 1 before the first step)
  long long* words;                   // [R] out: tokens fed to the next decoder step
  int* n_done;                        // *n_done += rows that finished in this launch
  float* tok_logp;                    // [R][max_len] or null: log-probability of the chosen token under the processed row
  float* rows_out;                    // [max_len][R][V] or null: the processed row
  const float* uniforms;              // [R][max_len] or null (greedy)
  long long* pos_out; int* ticket;    // advance: the LAST workgroup to finish writes *pos_out = pos + 1 (every workgroup has read pos by then)
};

__global__ __launch_bounds__(NT) void hf_sample_step_kernel(const HfSampleP p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_val[NT / 64]; __shared__ int s_idx[NT / 64];
  __shared__ float s_scan[NT / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int V = p.V;
  float* x = reinterpret_cast<float*>(smem);                 // [V] the row as the processors leave it
  int* l_seq = reinterpret_cast<int*>(x + V);                // [max_len] the row's history
  const long pos = p.pos[0];
  const int cur = (int)pos + 1;                              // ids so far; the column this launch writes
  if (pos >= 0 && cur < p.max_len) {                         // (uniform; a position outside the row writes nothing)
    // ---- 0. everything this workgroup reads, requested in batches: the row, its history, its flag
    const float* row = p.logits + (long)r * p.ld;
    long long* seq = p.seqs + (long)r * p.max_len;
    const bool fin = !p.unfinished[r];
    const float u = p.uniforms ? p.uniforms[(long)r * p.max_len + cur] : 0.f;
    for (int c = tid; c < p.max_len; c += NT) {
      const long long w = c < cur ? seq[c] : -1;
      l_seq[c] = (w >= 0 && w < V) ? (int)w : -1;            // (an id outside the row touches nothing below)
    }
    walk_row<NT>(row, V, [&](int w, float v) { x[w] = v; });
    __syncthreads();
    // ---- 1. repetition penalty, 2. no-repeat n-grams, 3. minimum length
    if (p.rep_penalty != 1.f) {
      hf_repetition_penalty<NT>(x, l_seq, cur, V, p.rep_penalty);
      __syncthreads();
    }
    if (p.ngram > 0 && cur >= p.ngram) {
      hf_ban_ngrams<NT>(x, l_seq, cur, V, p.ngram);
      __syncthreads();
    }
    if (cur < p.min_length) {
      if (tid == 0) hf_min_length(x, p.eos);
      __syncthreads();
    }
    // ---- 4. temperature (a division, as HF's), the row's arg-max
    float bv = -INFINITY; int bi = NO_CAND;
    for (int w = tid; w < V; w += NT) {
      float v = x[w];
      if (p.do_sample && p.temperature != 1.f) { v = v / p.temperature; x[w] = v; }      // (own entries only: no barrier needed)
      if (v > bv) { bv = v; bi = w; }                        // ascending index: ties keep the lowest
    }
    block_argmax<NT>(bv, bi, s_val, s_idx);
    const bool empty = bi == NO_CAND || !(bv > -INFINITY) || !(bv < INFINITY);     // no entry to choose from (all -inf / NaN), or an infinite one
    int it = bi == NO_CAND ? p.pad : bi;
    uint32_t thr = 0u;                                       // the smallest kept key (0: everything stays)
    if (p.do_sample && !empty) {
      // ---- 5. top-k: the key of the k-th largest value = the smallest m with fewer than k entries above it
      if (p.top_k > 0 && p.top_k < V) {
        const float k = (float)p.top_k;
        uint32_t lo = 0x007fffffu, hi = fkey(bv);            // key(-inf) .. key(row maximum)
        while (lo < hi) {                                    // (uniform: every thread holds the same reduction results)
          const uint32_t mid = lo + ((hi - lo) >> 1);
          float a = 0.f;
          for (int w = tid; w < V; w += NT) a += fkey(x[w]) > mid ? 1.f : 0.f;
          if (block_sum<NT>(a, s_val) < k) hi = mid; else lo = mid + 1;
        }
        thr = hi;
      }
      // ---- 6. top-p over the softmax of what top-k left: the smallest m whose mass of entries <= m exceeds (1 - p) * total
      if (p.top_p < 1.f) {
        auto below = [&](uint32_t m) {                       // mass of the kept entries with key <= m
          float a = 0.f;
          for (int w = tid; w < V; w += NT) { const uint32_t kx = fkey(x[w]); if (kx >= thr && kx <= m) a += expf(x[w] - bv); }
          return block_sum<NT>(a, s_val);
        };
        const uint32_t top = fkey(bv);
        const float limit = (1.f - p.top_p) * below(top);
        uint32_t lo = thr > 0x007fffffu ? thr : 0x007fffffu, hi = top;          // below(top) = total > limit: the maximum always stays
        while (lo < hi) {
          const uint32_t mid = lo + ((hi - lo) >> 1);
          if (below(mid) > limit) hi = mid; else lo = mid + 1;
        }
        thr = hi;
      }
      if (thr) {
        __syncthreads();
        for (int w = tid; w < V; w += NT) if (fkey(x[w]) < thr) x[w] = -INFINITY;
      }
    }
    __syncthreads();
    // ---- 7. the processed row leaves; total weight of the kept entries
    float part = 0.f;
    float* out = p.rows_out ? p.rows_out + ((long)cur * gridDim.x + r) * V : nullptr;
    for (int w = tid; w < V; w += NT) {
      const float v = x[w];
      if (out) out[w] = v;
      if (!empty) part += expf(v - bv);                      // (exp(-inf) = 0)
    }
    const float total = empty ? 1.f : block_sum<NT>(part, s_val);
    // ---- 8. the draw: inverse CDF over the kept entries in vocabulary order (a removed entry weighs exp(-inf) = 0)
    if (p.do_sample && !empty) it = draw_inverse_cdf<NT>(V, u, it, [&](int j) { return expf(x[j] - bv); }, s_scan, s_val, s_idx);
    // ---- 9. finished rows emit [PAD]; a row finishes when it emits [EOS]
    if (tid == 0) {
      float lp = empty ? 0.f : (x[it] - bv) - logf(total);
      if (fin) { it = p.pad; lp = 0.f; }
      else if (it == p.eos) { p.unfinished[r] = 0; atomicAdd(p.n_done, 1); }
      seq[cur] = it;
      p.words[r] = it;
      if (p.tok_logp) p.tok_logp[(long)r * p.max_len + cur] = lp;
    }
  }
  if (p.pos_out) advance_position(p.pos_out, p.ticket, pos);
}

}  // namespace

extern "C" {

int evk_hf_sample_step(const float* logits, int32_t ld, int32_t V, int32_t R, int32_t max_len, const int64_t* pos, int32_t eos, int32_t pad,
                       int32_t do_sample, float repetition_penalty, int32_t no_repeat_ngram, int32_t min_length, float temperature,
                       int32_t top_k, float top_p, int64_t* seqs, unsigned char* unfinished, int64_t* words, int32_t* n_done, float* tok_logp,
                       float* rows_out, const float* uniforms, int64_t* pos_advance, int32_t* ticket, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EVK_REQUIRE(logits && pos && seqs && unfinished && words && n_done && R > 0 && V > 0 && ld >= V && max_len > 1, "hf_sample_step: bad args");
  EVK_REQUIRE(V <= V_MAX, "hf_sample_step: V = %d exceeds %d (the row is kept in LDS)", V, V_MAX);
  EVK_REQUIRE(max_len <= LEN_MAX, "hf_sample_step: max_len = %d exceeds %d (the history is kept in LDS)", max_len, LEN_MAX);
  EVK_REQUIRE(eos >= 0 && eos < V && pad >= 0 && pad < V, "hf_sample_step: bad token ids");
  EVK_REQUIRE(repetition_penalty > 0.f, "hf_sample_step: repetition_penalty must be > 0 (got %g)", (double)repetition_penalty);
  EVK_REQUIRE(no_repeat_ngram >= 0 && no_repeat_ngram <= NGRAM_MAX, "hf_sample_step: no_repeat_ngram must be in [0, %d] (got %d)", NGRAM_MAX,
              no_repeat_ngram);
  EVK_REQUIRE(min_length >= 0, "hf_sample_step: min_length must be >= 0");
  EVK_REQUIRE(!do_sample || uniforms, "hf_sample_step: do_sample needs uniforms");
  EVK_REQUIRE(!do_sample || temperature > 0.f, "hf_sample_step: temperature must be > 0 (got %g)", (double)temperature);
  EVK_REQUIRE(!do_sample || top_k >= 0, "hf_sample_step: top_k must be >= 0 (got %d)", top_k);
  EVK_REQUIRE(!do_sample || (top_p > 0.f && top_p <= 1.f), "hf_sample_step: top_p must be in (0, 1] (got %g)", (double)top_p);
  EVK_REQUIRE(!pos_advance || ticket, "hf_sample_step: advancing the position needs a (zero-initialised) ticket word");
  const size_t lds = (size_t)V * 4 + (size_t)max_len * 4;
  HfSampleP p{logits, ld, V, max_len, eos, pad, do_sample ? 1 : 0, no_repeat_ngram, min_length, top_k, repetition_penalty, temperature, top_p,
              reinterpret_cast<const long long*>(pos), reinterpret_cast<long long*>(seqs), unfinished, reinterpret_cast<long long*>(words),
              n_done, tok_logp, rows_out, uniforms, reinterpret_cast<long long*>(pos_advance), ticket};
  ProfScope ps(EVK_FAM_NORM, s);
  hipLaunchKernelGGL(hf_sample_step_kernel, dim3(R), dim3(NT), lds, s, p);
  return evk_check_launch("hf_sample_step");
}

}  // extern "C"
