// beam.hip -- one kernel per generated token for ALL the beam bookkeeping of CaptionModel.beam_search / beam_step
// (modules/caption_model.py:51-106: candidate scores = running sum + log-prob, flat descending sort over beam x (V+1), top-beam,
// state / sequence reorder; :174-189: beams that emit [EOS] -- or every beam at the last position -- are recorded as finished
// with p = running sum and get -1000 on their running sum; modules/att_model.py:133-135: the best finished beam wins).
// The reference does this with a per-sample Python loop and .item() syncs; the first engine with ~15 torch glue ops per token
// inside the captured decode step (gather / where / max / index_copy kernels).  Here: one workgroup per sample --
//   1. every thread keeps the top-`beam` of its strided share of the beam x (V+1) candidates, `beam` rounds of a block arg-max
//      (ties -> lowest flat index, i.e. torch.sort(descending=True)'s order on distinct scores) pick the winners;
//   2. the sample's old sequences, cache row tables and relational-memory rows are staged in LDS and rewritten IN PLACE in the
//      winners' order (a sample's hypotheses only permute among themselves), the new token goes to position *pos;
//   3. finished-beam tracking and the -1000 penalty, the next step's input tokens.
#include <stdlib.h>
#include "decode_step.h"

namespace {

constexpr int KMAX = 8;

struct BeamP {
  const float* logp; int ld;          // [B*beam][ld] f32 log-probs of the step, V1 valid columns
  int V1, beam, max_len, eos, force_end;
  const long long* pos;               // device scalar: position being written
  float* beam_sum;                    // [B][beam] running sums (in / out)
  long long* beam_seq;                // [B][beam][max_len] (in place)
  float* best_p; long long* best_seq; // [B], [B][max_len]
  long long* words;                   // [B*beam] out: tokens fed to the next decoder step
  bf16_t* mem; int mem_row;           // relational-memory state [B*beam][mem_row] (in place) or null
  int* anc; int anc_cols;             // cache row table [B*beam][anc_cols] (in place) or null
  bf16_t* mem2;                       // optional second state row per hypothesis (same geometry as mem)
  long long* pos_out; int* ticket;    // advance: the LAST workgroup to finish writes *pos_out = pos + 1 (every workgroup has read pos by then)
};

// What evk_beam_step_opts adds (caption_model.py:148-150 previous-word constraint, :181-188 + :199 the sorted list of finished beams under
// utils.penalty_builder, :84-99 the log-probability rows every decision was taken from).  The kernels are templates over OPTS: the
// instantiation behind evk_beam_step carries none of this, neither as code nor as kernel arguments.
struct BeamOpts {
  int constraint, pad, R;             // mask the previous word's column at pos > 0; [PAD] id; R = B * beam rows of one history slab
  const double* len_div;              // [max_len] or null: list score = running sum / len_div[pos] (f64), null = the running sum itself
  double* fin_score; int* fin_len;    // [B][beam] finished list: score descending (ties: earlier entry first), length (0 = empty slot)
  long long* fin_seq; int* fin_anc;   // [B][beam][max_len] words (padded with `pad`) and, per position, the row that scored it (or null)
  float* hist;                        // [max_len][R][V1] or null: the rows of position pos as this step scanned them
};
template <bool OPTS> struct BeamArgs : BeamP {};
template <> struct BeamArgs<true> : BeamP { BeamOpts o; };

// ---- the tail of both step kernels: finished beams (best p so far; the earlier / lower beam index wins ties), the -1000 penalty, next
// tokens; with OPTS the finished hypotheses of this step enter the study's sorted list; the row table's next column, the position advance
template <bool OPTS>
__device__ __forceinline__ void beam_finish(const BeamArgs<OPTS>& p, int b, int tid, long pos, const float* win_v, const int* win_i,
                                            const long long* l_seq, const int* l_anc) {
  __shared__ int s_best;
  const int beam = p.beam, V1 = p.V1;
  if (tid == 0) {
    float pv = -INFINITY; int pi = -1;
    for (int j = 0; j < beam; ++j) {
      const int word = win_i[j] % V1;
      const bool end = p.force_end || word == p.eos;
      if (end && win_v[j] > pv) { pv = win_v[j]; pi = j; }
      p.beam_sum[b * beam + j] = win_v[j] - (end ? 1000.f : 0.f);
      p.words[b * beam + j] = word;
    }
    int take = -1;
    if (pi >= 0 && pv > p.best_p[b]) { p.best_p[b] = pv; take = pi; }
    s_best = take;
  }
  __syncthreads();
  if (s_best >= 0) {
    const int j = s_best, src = win_i[j] / V1;
    for (int c = tid; c < p.max_len; c += 256)
      p.best_seq[(long)b * p.max_len + c] = c == pos ? (long long)(win_i[j] % V1) : l_seq[src * p.max_len + c];
  }
  if constexpr (OPTS) {
    // thread 0 ranks the finished hypotheses of this step into the study's list, then every thread moves its columns of the list's rows
    __shared__ double f_sc[KMAX]; __shared__ int f_ln[KMAX]; __shared__ int f_src[KMAX];
    const BeamOpts& o = p.o;
    if (tid == 0) {
      for (int k = 0; k < beam; ++k) { f_sc[k] = o.fin_score[b * beam + k]; f_ln[k] = o.fin_len[b * beam + k]; f_src[k] = k; }
      const double div = (o.len_div && pos >= 0 && pos < p.max_len) ? o.len_div[pos] : 1.0;
      for (int j = 0; j < beam; ++j)
        if (p.force_end || win_i[j] % V1 == p.eos)
          list_insert(f_sc, f_ln, f_src, beam, o.len_div ? (double)win_v[j] / div : (double)win_v[j], (int)pos + 1, j);
      for (int k = 0; k < beam; ++k) { o.fin_score[b * beam + k] = f_sc[k]; o.fin_len[b * beam + k] = f_ln[k]; }
    }
    __syncthreads();
    // a fresh entry's row: the words of its source beam, the new word, [PAD]; per position the row that scored it
    list_move_rows<256>(o.fin_seq + (long)b * beam * p.max_len, f_src, beam, p.max_len, [&](int j, int c) {
      return c < pos ? l_seq[(win_i[j] / V1) * p.max_len + c] : c == pos ? (long long)(win_i[j] % V1) : (long long)o.pad;
    });
    if (o.fin_anc)
      list_move_rows<256>(o.fin_anc + (long)b * beam * p.max_len, f_src, beam, p.max_len, [&](int j, int c) {
        const int sb = win_i[j] / V1;
        return c < pos ? ((l_anc && c < p.anc_cols) ? l_anc[sb * p.anc_cols + c] : b * beam) : c == pos ? b * beam + sb : 0;
      });
  }
  if (p.pos_out) {
    // the next decoder step writes its keys / values at position pos + 1 of every hypothesis's OWN cache row: seed that column of the row
    // table here (it replaces an index_copy launch), then let the last workgroup advance the position (it replaces an add launch)
    if (p.anc && pos + 1 < p.anc_cols && tid < beam) p.anc[(long)(b * beam + tid) * p.anc_cols + pos + 1] = b * beam + tid;
    advance_position(p.pos_out, p.ticket, pos);
  }
}
// the sequences and the row table of the sample in the winners' order, the new token at position pos
__device__ __forceinline__ void beam_rewrite(const BeamP& p, int b, long pos, const int* win_i, const long long* l_seq, const int* l_anc) {
  const auto src_of = [&](int j) { return win_i[j] / p.V1; };
  rewrite_rows<256>(p.beam_seq + (long)b * p.beam * p.max_len, l_seq, p.beam, p.max_len, pos, src_of, [&](int j) { return win_i[j] % p.V1; });
  if (p.anc) rewrite_rows<256>(p.anc + (long)b * p.beam * p.anc_cols, l_anc, p.beam, p.anc_cols, -1, src_of, [](int) { return 0; });
}

template <bool OPTS>
__global__ __launch_bounds__(256) void beam_step_kernel(const BeamArgs<OPTS> p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float s_val[4]; __shared__ int s_idx[4];
  __shared__ float win_v[KMAX]; __shared__ int win_i[KMAX];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int beam = p.beam;
  const long pos = p.pos[0];
  // ---- 1. top-`beam` candidates: every thread keeps the best of its share, `beam` block rounds pick the winners.  With no comparable
  // candidate left (every log-probability of the sample NaN) slot r keeps ITS OWN hypothesis and emits token 0, as in the fast kernel
  CandList<KMAX> best;
  best.clear();
  for (int src = 0; src < beam; ++src) {
    const float base = p.beam_sum[b * beam + src];
    int prev = -1; float* hrow = nullptr;
    if constexpr (OPTS) {
      if (p.o.constraint && pos > 0 && pos < p.max_len) prev = (int)p.beam_seq[((long)b * beam + src) * p.max_len + pos - 1];
      if (p.o.hist && pos >= 0 && pos < p.max_len) hrow = p.o.hist + ((long)pos * p.o.R + b * beam + src) * p.V1;
    }
    walk_row<256>(p.logp + (long)(b * beam + src) * p.ld, p.V1, [&](int w, float lv) {
      if constexpr (OPTS) {
        if (w == prev) lv = -INFINITY;
        if (hrow) hrow[w] = lv;
      }
      best.insert(base + lv, src * p.V1 + w, beam);
    });
  }
  pick_rounds<256>(best, beam, p.V1, s_val, s_idx, win_v, win_i);
  // ---- 2. stage the sample's rows, rewrite them in the winners' order
  long long* seq = p.beam_seq + (long)b * beam * p.max_len;
  long long* l_seq = reinterpret_cast<long long*>(smem);                               // [beam][max_len]
  int* l_anc = reinterpret_cast<int*>(l_seq + (size_t)beam * p.max_len);               // [beam][anc_cols]
  uint32_t* l_mem = reinterpret_cast<uint32_t*>(l_anc + (size_t)beam * (p.anc ? p.anc_cols : 0));   // [beam][mem_row / 2]
  for (int i = tid; i < beam * p.max_len; i += 256) l_seq[i] = seq[i];
  if (p.anc) for (int i = tid; i < beam * p.anc_cols; i += 256) l_anc[i] = p.anc[(long)b * beam * p.anc_cols + i];
  const int mw = p.mem_row / 2;
  if (p.mem) {
    const uint32_t* gm = reinterpret_cast<const uint32_t*>(p.mem + (long)b * beam * p.mem_row);
    for (int i = tid; i < beam * mw; i += 256) l_mem[i] = gm[i];
  }
  __syncthreads();
  beam_rewrite(p, b, pos, win_i, l_seq, l_anc);
  if (p.mem) {
    uint32_t* gm = reinterpret_cast<uint32_t*>(p.mem + (long)b * beam * p.mem_row);
    for (int i = tid; i < beam * mw; i += 256) {
      const int j = i / mw, c = i - j * mw;
      gm[i] = l_mem[(win_i[j] / p.V1) * mw + c];
    }
  }
  if (p.mem2) {                         // second state: through the same staging buffer, after the first has left it
    __syncthreads();
    uint32_t* gm = reinterpret_cast<uint32_t*>(p.mem2 + (long)b * beam * p.mem_row);
    for (int i = tid; i < beam * mw; i += 256) l_mem[i] = gm[i];
    __syncthreads();
    for (int i = tid; i < beam * mw; i += 256) {
      const int j = i / mw, c = i - j * mw;
      gm[i] = l_mem[(win_i[j] / p.V1) * mw + c];
    }
  }
  // ---- 3. finished beams, the -1000 penalty, next tokens, the position advance
  beam_finish<OPTS>(p, b, tid, pos, win_v, win_i, l_seq, p.anc ? l_anc : nullptr);
}

// The same step with ONE memory round trip in front of the selection: the sample's state rows (sequences, cache row table, memory) and
// all beam x (V+1) candidates are requested together -- each wave owns the candidates of one source beam in registers (V + 1 <= 1536) --,
// the top-`beam` of every source row are found by `beam` rounds of a wave arg-max and merged by wave 0 (beam x beam candidates).  The
// kernel above walks the candidates beam by beam (a round trip each), keeps a sorted list per thread and stages the state afterwards
// (two more round trips): 29 us of a ~400 us token step; this one takes a third of that.  Same results bit for bit: the order (score,
// then lowest flat index) is total.
constexpr int CMAX = 24;        // candidates per lane and source row

// arg-max (value, then LOWEST index) over the 64 lanes, result in every lane: four DPP exchanges inside the rows of 16 lanes (a few cycles
// each; __shfl_xor goes through the LDS crossbar, ~100 cycles per dependent step: 12 of them per round were most of this kernel), then the
// four row results are read as scalars
template <int CTRL>
__device__ __forceinline__ void dpp_argmax_step(float& v, int& i) {
  const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
  const int oi = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xF, 0xF, true);
  if (better(ov, oi, v, i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
  dpp_argmax_step<0xB1>(v, i);       // quad_perm [1,0,3,2]
  dpp_argmax_step<0x4E>(v, i);       // quad_perm [2,3,0,1]
  dpp_argmax_step<0x141>(v, i);      // row_half_mirror
  dpp_argmax_step<0x140>(v, i);      // row_mirror: every lane of a row holds the row's result
  float bv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
  int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
  for (int r = 1; r < 4; ++r) {
    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16 * r));
    const int oi = __builtin_amdgcn_readlane(i, 16 * r);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  v = bv; i = bi;
}

template <bool OPTS>
__global__ __launch_bounds__(256) void beam_step_fast_kernel(const BeamArgs<OPTS> p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float c_val[KMAX * KMAX]; __shared__ int c_idx[KMAX * KMAX];
  __shared__ float win_v[KMAX]; __shared__ int win_i[KMAX];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int beam = p.beam, V1 = p.V1;
  const long pos = p.pos[0];
  // ---- 0. everything this workgroup reads, requested at once
  long long* seq = p.beam_seq + (long)b * beam * p.max_len;
  long long* l_seq = reinterpret_cast<long long*>(smem);                               // [beam][max_len]
  int* l_anc = reinterpret_cast<int*>(l_seq + (size_t)beam * p.max_len);               // [beam][anc_cols]
  uint32_t* l_mem = reinterpret_cast<uint32_t*>(l_anc + (size_t)beam * (p.anc ? p.anc_cols : 0));   // [beam][mem_row / 2]
  const int mw = p.mem_row / 2;
  uint32_t* l_mem2 = l_mem + (size_t)beam * (p.mem ? mw : 0);
  float x[2][CMAX];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int src = wave + 4 * u;
    const float* row = p.logp + (long)(b * beam + min(src, beam - 1)) * p.ld;
#pragma unroll
    for (int i = 0; i < CMAX; ++i) { const int c = lane + 64 * i; x[u][i] = (src < beam && c < V1) ? row[c] : -INFINITY; }
    if constexpr (OPTS) {
      // the previous word's column is masked and the row goes to the history as it is scanned (no launch, one more write stream)
      if (src < beam) {
        int prev = -1;
        if (p.o.constraint && pos > 0 && pos < p.max_len) prev = (int)seq[(long)src * p.max_len + pos - 1];
        float* hrow = (p.o.hist && pos >= 0 && pos < p.max_len) ? p.o.hist + ((long)pos * p.o.R + b * beam + src) * V1 : nullptr;
#pragma unroll
        for (int i = 0; i < CMAX; ++i) {
          const int c = lane + 64 * i;
          if (c == prev) x[u][i] = -INFINITY;
          if (hrow && c < V1) hrow[c] = x[u][i];
        }
      }
    }
  }
  float base[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) base[u] = p.beam_sum[b * beam + min(wave + 4 * u, beam - 1)];
  // state rows -> LDS in 16-byte pieces, eight per thread in flight (a word-by-word loop of unknown trip count is a chain of dependent
  // round trips: 24 of them for the 24 KB of f32 memory rows were most of this kernel's first version)
  auto stage = [&](void* dst, const void* src, int nbytes) {
    if ((nbytes & 15) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
      const int n4 = nbytes >> 4;
      for (int base = 0; base < n4; base += 256 * 8) {
        uint4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = base + tid + 256 * u; if (i < n4) t[u] = reinterpret_cast<const uint4*>(src)[i]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int i = base + tid + 256 * u; if (i < n4) reinterpret_cast<uint4*>(dst)[i] = t[u]; }
      }
    } else {
      for (int i = tid; i < (nbytes >> 2); i += 256) reinterpret_cast<uint32_t*>(dst)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    }
  };
  stage(l_seq, seq, beam * p.max_len * 8);
  if (p.anc) stage(l_anc, p.anc + (long)b * beam * p.anc_cols, beam * p.anc_cols * 4);
  if (p.mem) stage(l_mem, p.mem + (long)b * beam * p.mem_row, beam * p.mem_row * 2);
  if (p.mem2) stage(l_mem2, p.mem2 + (long)b * beam * p.mem_row, beam * p.mem_row * 2);
  // ---- 1. top-`beam` of every source row (wave = source beam, + 4 for beams 4 .. 7)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int src = wave + 4 * u;
    if (src >= beam) continue;                       // (wave-uniform)
#pragma unroll
    for (int i = 0; i < CMAX; ++i) x[u][i] += base[u];            // -inf stays -inf
    for (int r = 0; r < beam; ++r) {
      float bv = -INFINITY; int bi = NO_CAND;
#pragma unroll
      for (int i = 0; i < CMAX; ++i) if (x[u][i] > bv) { bv = x[u][i]; bi = src * V1 + lane + 64 * i; }      // ascending index: ties keep the lowest
      wave_argmax(bv, bi);
      if (lane == 0) { c_val[src * beam + r] = bv; c_idx[src * beam + r] = bi; }
      const int wc = bi - src * V1;                  // the winner's column: its owner retires it
      if ((wc & 63) == lane) {
#pragma unroll
        for (int i = 0; i < CMAX; ++i) if (i == (wc >> 6)) x[u][i] = -INFINITY;
      }
    }
  }
  __syncthreads();
  // ---- 2. merge the beam x beam survivors (wave 0)
  if (wave == 0) {
    float v = lane < beam * beam ? c_val[lane] : -INFINITY;
    int id = lane < beam * beam ? c_idx[lane] : NO_CAND;
    for (int r = 0; r < beam; ++r) {
      float bv = v; int bi = id;
      wave_argmax(bv, bi);
      // No comparable candidate left (every log-probability of the sample NaN or -inf: the forward guard only scans the trunk output): the
      // sentinel index would address LDS rows beyond the sample's beams below -- slot r then keeps ITS OWN hypothesis and emits token 0 ([PAD]),
      // a defined state instead of garbage.
      if (lane == 0) { win_v[r] = bv; win_i[r] = bi == NO_CAND ? r * V1 : bi; }
      if (id == bi) { v = -INFINITY; id = NO_CAND; }
    }
  }
  __syncthreads();
  // ---- 3. rewrite the sample's rows in the winners' order (a sample's hypotheses only permute among themselves)
  beam_rewrite(p, b, pos, win_i, l_seq, l_anc);
  auto permute_rows = [&](void* g, const uint32_t* l) {          // row j <- staged row of its source beam; rows that stay are not rewritten
    if ((mw & 3) == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(l)) & 15) == 0) {
      const int w4 = mw >> 2;
      for (int i = tid; i < beam * w4; i += 256) {
        const int j = i / w4, c = i - j * w4;
        const int src = win_i[j] / V1;
        if (src != j) reinterpret_cast<uint4*>(g)[i] = reinterpret_cast<const uint4*>(l)[src * w4 + c];
      }
    } else {
      for (int i = tid; i < beam * mw; i += 256) {
        const int j = i / mw, c = i - j * mw;
        const int src = win_i[j] / V1;
        if (src != j) reinterpret_cast<uint32_t*>(g)[i] = l[src * mw + c];
      }
    }
  };
  if (p.mem) permute_rows(p.mem + (long)b * beam * p.mem_row, l_mem);
  if (p.mem2) permute_rows(p.mem2 + (long)b * beam * p.mem_row, l_mem2);
  // ---- 4. finished beams, the -1000 penalty, next tokens, the position advance
  beam_finish<OPTS>(p, b, tid, pos, win_v, win_i, l_seq, p.anc ? l_anc : nullptr);
}

// out[b * take + k][t][:] = hist[t][fin_anc[b][k][t]][:] for t < fin_len[b][k], zeros beyond: the seqLogprobs rows of the returned
// hypotheses (att_model.py:131 / :135), read once after the search.  Pure copy: one workgroup per (position, output row).
struct GatherP { const float* hist; const int* fin_anc; const int* fin_len; float* out; int beam, take, max_len, V1, R; };
__global__ __launch_bounds__(256) void beam_gather_kernel(const GatherP p) {
  const int t = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const int e = (row / p.take) * p.beam + row % p.take;               // list entry
  const int a = p.fin_anc[(long)e * p.max_len + t];
  const bool live = t < p.fin_len[e] && a >= 0 && a < p.R;
  float* dst = p.out + ((long)row * p.max_len + t) * p.V1;
  const float* src = p.hist + ((long)t * p.R + (live ? a : 0)) * p.V1;
  if ((p.V1 & 3) == 0) {                                              // every row starts on a 16-byte boundary
    const int n4 = p.V1 >> 2;
    for (int i = tid; i < n4; i += 256) reinterpret_cast<float4*>(dst)[i] = live ? reinterpret_cast<const float4*>(src)[i] : float4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int i0 = tid; i0 < p.V1; i0 += 256 * 4) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int i = i0 + 256 * u; v[u] = (live && i < p.V1) ? src[i] : 0.f; }
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int i = i0 + 256 * u; if (i < p.V1) dst[i] = v[u]; }
    }
  }
}

int launch_beam_step(const BeamP& p, const BeamOpts* o, int B, hipStream_t s, const char* what) {
  EVK_REQUIRE(p.logp && p.pos && p.beam_sum && p.beam_seq && p.best_p && p.best_seq && p.words && B > 0 && p.V1 > 0 && p.ld >= p.V1 && p.max_len > 0,
              "%s: bad args", what);
  EVK_REQUIRE(p.beam >= 1 && p.beam <= KMAX && p.beam <= p.V1, "%s: beam must be in [1, %d]", what, KMAX);
  EVK_REQUIRE((!p.mem || (p.mem_row > 0 && p.mem_row % 2 == 0)) && (!p.anc || p.anc_cols > 0), "%s: bad state geometry", what);
  EVK_REQUIRE(!p.pos_out || p.ticket, "%s: advancing the position needs a (zero-initialised) ticket word", what);
  EVK_REQUIRE(!p.mem2 || p.mem, "%s: mem2 needs mem", what);
  static const int fast_on = evk_tunable("EVK_BEAM_STEP_FAST", 1);
  const bool fast = fast_on && p.V1 <= CMAX * 64;
  const size_t lds = (size_t)p.beam * p.max_len * 8 + (p.anc ? (size_t)p.beam * p.anc_cols * 4 : 0) + (p.mem ? (size_t)p.beam * p.mem_row * 2 : 0) +
                     (fast && p.mem2 ? (size_t)p.beam * p.mem_row * 2 : 0);
  EVK_REQUIRE(lds <= 60000, "%s: %zu bytes of per-sample state do not fit the staging buffer", what, lds);
  ProfScope ps(EVK_FAM_NORM, s);
  if (o) {
    BeamArgs<true> a; static_cast<BeamP&>(a) = p; a.o = *o;
    if (fast) hipLaunchKernelGGL(beam_step_fast_kernel<true>, dim3(B), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(beam_step_kernel<true>, dim3(B), dim3(256), lds, s, a);
  } else {
    BeamArgs<false> a; static_cast<BeamP&>(a) = p;
    if (fast) hipLaunchKernelGGL(beam_step_fast_kernel<false>, dim3(B), dim3(256), lds, s, a);
    else hipLaunchKernelGGL(beam_step_kernel<false>, dim3(B), dim3(256), lds, s, a);
  }
  return evk_check_launch(what);
}

}  // namespace

extern "C" {

int evk_beam_step(const float* logp, int32_t ld, int32_t V1, int32_t beam, int32_t B, int32_t max_len, const int64_t* pos, int32_t eos,
                  int32_t force_end, float* beam_sum, int64_t* beam_seq, float* best_p, int64_t* best_seq, int64_t* words, void* mem,
                  int32_t mem_row, int32_t* anc, int32_t anc_cols, int64_t* pos_advance, int32_t* ticket, void* mem2, evk_stream_t stream) {
  BeamP p{logp, ld, V1, beam, max_len, eos, force_end, reinterpret_cast<const long long*>(pos), beam_sum, reinterpret_cast<long long*>(beam_seq),
          best_p, reinterpret_cast<long long*>(best_seq), reinterpret_cast<long long*>(words), (bf16_t*)mem, mem_row, anc, anc_cols,
          (bf16_t*)mem2, reinterpret_cast<long long*>(pos_advance), ticket};
  return launch_beam_step(p, nullptr, B, reinterpret_cast<hipStream_t>(stream), "beam_step");
}

int evk_beam_step_opts(const float* logp, int32_t ld, int32_t V1, int32_t beam, int32_t B, int32_t max_len, const int64_t* pos, int32_t eos,
                       int32_t force_end, float* beam_sum, int64_t* beam_seq, float* best_p, int64_t* best_seq, int64_t* words, void* mem,
                       int32_t mem_row, int32_t* anc, int32_t anc_cols, int64_t* pos_advance, int32_t* ticket, void* mem2, int32_t pad,
                       int32_t decoding_constraint, const double* len_div, double* fin_score, int32_t* fin_len, int64_t* fin_seq,
                       int32_t* fin_anc, float* hist, evk_stream_t stream) {
  EVK_REQUIRE(fin_score && fin_len && fin_seq, "beam_step_opts: the finished list (score, length, sequence) is required");
  EVK_REQUIRE(B > 0 && beam >= 1 && (int64_t)B * beam <= INT32_MAX / 2, "beam_step_opts: bad args");
  BeamP p{logp, ld, V1, beam, max_len, eos, force_end, reinterpret_cast<const long long*>(pos), beam_sum, reinterpret_cast<long long*>(beam_seq),
          best_p, reinterpret_cast<long long*>(best_seq), reinterpret_cast<long long*>(words), (bf16_t*)mem, mem_row, anc, anc_cols,
          (bf16_t*)mem2, reinterpret_cast<long long*>(pos_advance), ticket};
  BeamOpts o{decoding_constraint != 0, pad, B * beam, len_div, fin_score, fin_len, reinterpret_cast<long long*>(fin_seq), fin_anc, hist};
  return launch_beam_step(p, &o, B, reinterpret_cast<hipStream_t>(stream), "beam_step_opts");
}

int evk_beam_gather_logprobs(const float* hist, const int32_t* fin_anc, const int32_t* fin_len, float* out, int32_t B, int32_t beam,
                             int32_t take, int32_t max_len, int32_t V1, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EVK_REQUIRE(hist && fin_anc && fin_len && out && B > 0 && V1 > 0 && max_len > 0, "beam_gather_logprobs: bad args");
  EVK_REQUIRE(beam >= 1 && beam <= KMAX && take >= 1 && take <= beam, "beam_gather_logprobs: take must be in [1, beam], beam in [1, %d]", KMAX);
  EVK_REQUIRE((int64_t)B * take <= 65535, "beam_gather_logprobs: %lld output rows exceed the grid", (long long)B * take);
  GatherP p{hist, fin_anc, fin_len, out, beam, take, max_len, V1, B * beam};
  ProfScope ps(EVK_FAM_NORM, s);
  hipLaunchKernelGGL(beam_gather_kernel, dim3(max_len, B * take), dim3(256), 0, s, p);
  return evk_check_launch("beam_gather_logprobs");
}

}  // extern "C"
