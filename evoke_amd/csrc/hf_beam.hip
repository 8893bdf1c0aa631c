// hf_beam.hip -- one kernel per generated token for ALL the beam bookkeeping of the distilgpt2 backend's search: what Hugging Face's
// classic BeamSearchScorer does between two decoder steps at length_penalty 1, early_stopping False (language_model.py:271-280 hands the
// search to `generate`; oracle/gpt2.py:120-186 restates it).  The first engine did this on the host: two device -> host copies per
// token, a Python double loop over studies x 2 * num_beams candidates, index_select over every self-attention cache.  Here: one
// workgroup per study --
//   1. candidate = running score of the source beam + log-probability (f32 add); every thread keeps the top 2 * nb of its strided share
//      of the nb x V candidates, 2 * nb rounds of a block arg-max pick them in descending order (ties -> lowest flat index);
//   2. thread 0 walks the ranks: an [EOS] candidate at rank < nb enters the study's sorted hypothesis list with score sum / cur_len (f64),
//      an [EOS] candidate at rank >= nb is skipped, the first nb other candidates are the next beams; then the done flag;
//   3. the study's sequences and cache row tables are staged in LDS and rewritten IN PLACE in the winners' order, the new token goes to
//      column *pos + 1, the row table's next column is seeded, and the last workgroup to finish advances the position.
// A study that is done emits [PAD] from its first row for ever and never touches its list again, so steps issued after every study is
// done change nothing that is returned.
// evk_hf_beam_step_opts is the same kernel body (a template parameter switches the additions on) with what `generate` adds to a beam search
// when it is asked for them: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinLengthLogitsProcessor on the
// log-probability rows of the running beams, each from its own history, before the candidates are formed (a pre-pass that edits `logp` in
// place), and the scorer's length_penalty (a host-computed table of divisors cur_len ** length_penalty) and early_stopping.
#include <stdlib.h>
#include "common.h"
#include "decode_step.h"

namespace {

constexpr int NBMAX = 8;

struct HfBeamP {
  const float* logp; int ld;           // [B*nb][ld] f32 log-probs of the step, V valid columns
  int V, nb, max_len, eos, pad, force_end;
  const long long* pos;                // device scalar: last filled column of seqs (cur_len = *pos + 1 generated tokens after this step)
  float* scores;                       // [B][nb] running sums (in / out)
  long long* seqs;                     // [B*nb][max_len] (in place), column 0 = [BOS]
  long long* words;                    // [B*nb] out: tokens fed to the next decoder step
  int* anc; int anc_cols;              // cache row table [B*nb][anc_cols] (in place) or null
  double* hyp_score; int* hyp_len;     // [B][nb] sorted hypothesis list: score descending (ties: earlier entry first), columns (0 = empty)
  long long* hyp_seq;                  // [B][nb][max_len] with the leading [BOS], padded with `pad`
  unsigned char* done; int* n_done;    // [B] flags (in / out); *n_done += studies that became done in this launch
  long long* pos_out; int* ticket;     // the LAST workgroup to finish writes *pos_out = pos + 1 (every workgroup has read pos by then)
  static constexpr bool kOpts = false;
};
struct HfBeamOptsP : HfBeamP {         // what evk_hf_beam_step_opts adds
  const double* len_div;               // [max_len + 1] divisor of a hypothesis that ends at cur_len, or null (= cur_len)
  float rep_penalty;                   // (logp is written: the processors edit the rows of a study that is not done in place)
  int ctl;                             // no_repeat_ngram_size | early_stopping << 4 | min(min_length, max_len) << 8 (one word: scalar registers are short)
  static constexpr bool kOpts = true;
};

template <int K2, class P>             // K2: capacity of a thread's candidate list, >= 2 * nb; P: HfBeamP or HfBeamOptsP
__global__ __launch_bounds__(256) void hf_beam_step_kernel(const P p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_val[4]; __shared__ int s_idx[4];
  __shared__ float win_v[2 * NBMAX]; __shared__ int win_i[2 * NBMAX];
  __shared__ float nx_sc[NBMAX]; __shared__ int nx_tok[NBMAX]; __shared__ int nx_src[NBMAX];
  __shared__ double f_sc[NBMAX]; __shared__ int f_ln[NBMAX]; __shared__ int f_src[NBMAX];
  __shared__ int s_list;               // the list's rows move in this launch
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nb = p.nb, V = p.V, k2 = 2 * nb;
  const long pos = p.pos[0];
  const bool was_done = p.done[b] != 0;                       // (block-uniform)
  // ---- 0. the study's rows -> LDS
  long long* seq = p.seqs + (long)b * nb * p.max_len;
  long long* l_seq = reinterpret_cast<long long*>(smem);                               // [nb][max_len]
  int* l_anc = reinterpret_cast<int*>(l_seq + (size_t)nb * p.max_len);                 // [nb][anc_cols]
  for (int i = tid; i < nb * p.max_len; i += 256) l_seq[i] = seq[i];
  if (p.anc) for (int i = tid; i < nb * p.anc_cols; i += 256) l_anc[i] = p.anc[(long)b * nb * p.anc_cols + i];
  if constexpr (P::kOpts) {
    // ---- 0b. the logits processors in HF's order on the rows of the nb running beams, each from its own history l_seq[j][0 .. cur - 1]
    if (!was_done) {                                           // (block-uniform, like every condition around a barrier below)
      __syncthreads();                                         // the histories are in LDS
      const int ml = p.max_len, cur = min((int)pos + 1, ml);      // ids so far, [BOS] included
      float* rows = const_cast<float*>(p.logp) + (long)b * nb * p.ld;
      if (p.rep_penalty != 1.f) {
        for (int j = 0; j < nb; ++j) hf_repetition_penalty<256>(rows + (long)j * p.ld, l_seq + j * ml, cur, V, p.rep_penalty);
        __syncthreads();                                       // a ban below must not be overwritten by a penalty's read-modify-write
      }
      const int g = p.ctl & 15;
      if (g > 0 && cur >= g)
        for (int j = 0; j < nb; ++j) hf_ban_ngrams<256>(rows + (long)j * p.ld, l_seq + j * ml, cur, V, g);
      if (cur < (p.ctl >> 8) && tid < nb) hf_min_length(rows + (long)tid * p.ld, p.eos);
      __syncthreads();                                         // the rows are re-read by this workgroup only
    }
  }
  if (!was_done) {
    // ---- 1. the 2 * nb best candidates, descending (no comparable candidate left: rank r takes source beam 0, token r < V, at -inf)
    CandList<K2> best;
    best.clear();
    for (int src = 0; src < nb; ++src) {
      const float base = p.scores[b * nb + src];
      walk_row<256>(p.logp + (long)(b * nb + src) * p.ld, V, [&](int w, float lv) { best.insert(base + lv, src * V + w, k2); });
    }
    pick_rounds<256>(best, k2, 1, s_val, s_idx, win_v, win_i);
  }
  // ---- 2. the rank walk (thread 0): hypothesis list, next beams, done flag
  if (tid == 0) {
    int moved = 0;
    if (was_done) {
      for (int k = 0; k < nb; ++k) { nx_sc[k] = 0.f; nx_tok[k] = p.pad; nx_src[k] = 0; }
    } else {
      double cur_len = (double)(pos + 1);                      // what a sum is divided by: cur_len ** length_penalty
      if constexpr (P::kOpts) { if (p.len_div) cur_len = p.len_div[pos + 1]; }
      int nx_rank[NBMAX];
      for (int k = 0; k < nb; ++k) { f_sc[k] = p.hyp_score[b * nb + k]; f_ln[k] = p.hyp_len[b * nb + k]; f_src[k] = k; }
      // the study's list in LDS; a fresh entry is named by its candidate's rank, its length is pos + 2 columns
      auto insert = [&](double s, int rank) { if (list_insert(f_sc, f_ln, f_src, nb, s, (int)pos + 2, rank)) moved = 1; };
      int k = 0;
      for (int rank = 0; rank < k2 && k < nb; ++rank) {
        const int src = win_i[rank] / V, tok = win_i[rank] - src * V;
        if (tok == p.eos) {
          if (rank < nb) insert((double)win_v[rank] / cur_len, rank);
          continue;
        }
        nx_sc[k] = win_v[rank]; nx_tok[k] = tok; nx_src[k] = src; nx_rank[k] = rank;
        ++k;
      }
      for (; k < nb; ++k) { nx_sc[k] = -INFINITY; nx_tok[k] = p.pad; nx_src[k] = 0; nx_rank[k] = 0; }     // (V >= 2 * nb: never taken on finite rows)
      bool now_done = f_ln[nb - 1] != 0 && f_sc[nb - 1] >= (double)win_v[0] / cur_len;
      if constexpr (P::kOpts) { if (p.ctl & 16) now_done = f_ln[nb - 1] != 0; }
      if (now_done) { p.done[b] = 1; atomicAdd(p.n_done, 1); }
      else if (p.force_end)
        for (int j = 0; j < nb; ++j) insert((double)nx_sc[j] / cur_len, nx_rank[j]);
      if (moved) for (int j = 0; j < nb; ++j) { p.hyp_score[b * nb + j] = f_sc[j]; p.hyp_len[b * nb + j] = f_ln[j]; }
    }
    s_list = moved;
  }
  __syncthreads();
  // ---- 3. the list's rows follow: a fresh entry is its source beam's row, the new token in column pos + 1, [PAD] beyond
  if (s_list)
    list_move_rows<256>(p.hyp_seq + (long)b * nb * p.max_len, f_src, nb, p.max_len, [&](int rank, int c) {
      const int src = win_i[rank] / V;
      return c <= pos ? l_seq[src * p.max_len + c] : c == pos + 1 ? (long long)(win_i[rank] - src * V) : (long long)p.pad;
    });
  // ---- 4. the study's rows in the winners' order, the new token in column pos + 1; the next decoder step writes its keys / values at
  // position pos + 1 of every hypothesis's OWN cache row
  const auto src_of = [&](int j) { return nx_src[j]; };
  rewrite_rows<256>(seq, l_seq, nb, p.max_len, pos + 1, src_of, [&](int j) { return nx_tok[j]; });
  if (p.anc) rewrite_rows<256>(p.anc + (long)b * nb * p.anc_cols, l_anc, nb, p.anc_cols, pos + 1, src_of, [&](int j) { return b * nb + j; });
  if (tid < nb) { p.scores[b * nb + tid] = nx_sc[tid]; p.words[b * nb + tid] = nx_tok[tid]; }
  if (p.pos_out) advance_position(p.pos_out, p.ticket, pos);
}

}  // namespace

// argument checks shared by the two entry points -> staging bytes, or -1 (evk_last_error says why)
static long hf_beam_check(const float* logp, int32_t ld, int32_t V, int32_t nb, int32_t B, int32_t max_len, const int64_t* pos, float* scores,
                          int64_t* seqs, int64_t* words, int32_t* anc, int32_t anc_cols, double* hyp_score, int32_t* hyp_len, int64_t* hyp_seq,
                          unsigned char* done, int32_t* n_done, int64_t* pos_advance, int32_t* ticket) {
  EVK_REQUIRE(nb >= 1 && nb <= NBMAX, "hf_beam_step: nb must be in [1, %d] (got %d)", NBMAX, nb);
  EVK_REQUIRE(V >= 2 * nb && (int64_t)nb * V < INT32_MAX, "hf_beam_step: V=%d must hold 2 * nb = %d candidates", V, 2 * nb);
  EVK_REQUIRE(ld >= V, "hf_beam_step: ld=%d < V=%d", ld, V);
  EVK_REQUIRE(logp && pos && scores && seqs && words && hyp_score && hyp_len && hyp_seq && done && n_done && B > 0 && max_len > 1,
              "hf_beam_step: null/empty");
  EVK_REQUIRE((int64_t)B * nb * (int64_t)max_len < INT32_MAX && (!anc || anc_cols > 0), "hf_beam_step: bad state geometry");
  EVK_REQUIRE(!pos_advance || ticket, "hf_beam_step: advancing the position needs a (zero-initialised) ticket word");
  const size_t lds = (size_t)nb * max_len * 8 + (anc ? (size_t)nb * anc_cols * 4 : 0);
  EVK_REQUIRE(lds <= 48000, "hf_beam_step: %zu bytes of per-study state do not fit the staging buffer", lds);
  return (long)lds;
}

template <class P>
static void hf_beam_launch(const P& p, int nb, int B, size_t lds, hipStream_t s) {
  if (nb <= 2) hipLaunchKernelGGL((hf_beam_step_kernel<4, P>), dim3(B), dim3(256), lds, s, p);
  else if (nb <= 4) hipLaunchKernelGGL((hf_beam_step_kernel<8, P>), dim3(B), dim3(256), lds, s, p);
  else hipLaunchKernelGGL((hf_beam_step_kernel<16, P>), dim3(B), dim3(256), lds, s, p);
}

extern "C" {

int evk_hf_beam_step(const float* logp, int32_t ld, int32_t V, int32_t nb, int32_t B, int32_t max_len, const int64_t* pos, int32_t eos,
                     int32_t pad, int32_t force_end, float* scores, int64_t* seqs, int64_t* words, int32_t* anc, int32_t anc_cols,
                     double* hyp_score, int32_t* hyp_len, int64_t* hyp_seq, unsigned char* done, int32_t* n_done, int64_t* pos_advance,
                     int32_t* ticket, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long lds = hf_beam_check(logp, ld, V, nb, B, max_len, pos, scores, seqs, words, anc, anc_cols, hyp_score, hyp_len, hyp_seq, done, n_done,
                                 pos_advance, ticket);
  if (lds < 0) return -1;
  HfBeamP p{logp, ld, V, nb, max_len, eos, pad, force_end, reinterpret_cast<const long long*>(pos), scores, reinterpret_cast<long long*>(seqs),
            reinterpret_cast<long long*>(words), anc, anc_cols, hyp_score, hyp_len, reinterpret_cast<long long*>(hyp_seq), done, n_done,
            reinterpret_cast<long long*>(pos_advance), ticket};
  ProfScope ps(EVK_FAM_NORM, s);
  hf_beam_launch(p, nb, B, (size_t)lds, s);
  return evk_check_launch("hf_beam_step");
}

int evk_hf_beam_step_opts(float* logp, int32_t ld, int32_t V, int32_t nb, int32_t B, int32_t max_len, const int64_t* pos, int32_t eos,
                          int32_t pad, int32_t force_end, float* scores, int64_t* seqs, int64_t* words, int32_t* anc, int32_t anc_cols,
                          double* hyp_score, int32_t* hyp_len, int64_t* hyp_seq, unsigned char* done, int32_t* n_done, int64_t* pos_advance,
                          int32_t* ticket, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t min_length, const double* len_div,
                          int32_t early_stopping, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EVK_REQUIRE(repetition_penalty > 0.f, "hf_beam_step_opts: repetition_penalty must be > 0 (got %g)", (double)repetition_penalty);
  EVK_REQUIRE(no_repeat_ngram_size >= 0 && no_repeat_ngram_size <= NGRAM_MAX, "hf_beam_step_opts: no_repeat_ngram_size must be in [0, %d] (got %d)",
              NGRAM_MAX, no_repeat_ngram_size);
  EVK_REQUIRE(min_length >= 0, "hf_beam_step_opts: min_length must be >= 0 (got %d)", min_length);
  const long lds = hf_beam_check(logp, ld, V, nb, B, max_len, pos, scores, seqs, words, anc, anc_cols, hyp_score, hyp_len, hyp_seq, done, n_done,
                                 pos_advance, ticket);
  if (lds < 0) return -1;
  EVK_REQUIRE(eos >= 0 && eos < V, "hf_beam_step_opts: eos=%d outside the %d valid columns", eos, V);
  HfBeamOptsP p{{logp, ld, V, nb, max_len, eos, pad, force_end, reinterpret_cast<const long long*>(pos), scores, reinterpret_cast<long long*>(seqs),
                 reinterpret_cast<long long*>(words), anc, anc_cols, hyp_score, hyp_len, reinterpret_cast<long long*>(hyp_seq), done, n_done,
                 reinterpret_cast<long long*>(pos_advance), ticket},
                len_div, repetition_penalty, no_repeat_ngram_size | (early_stopping ? 16 : 0) | (min_length < max_len ? min_length : max_len) << 8};
  ProfScope ps(EVK_FAM_NORM, s);
  hf_beam_launch(p, nb, B, (size_t)lds, s);
  return evk_check_launch("hf_beam_step_opts");
}

}  // extern "C"
