// decode_attn_wide.hip -- single-query attention of the incremental decode step for head sizes 128 and 256 (the EVOKE YAML decoder sizes:
// 2048 wide, 8 heads), the counterpart of decode_attn_kernel in norm.hip, which is hard-wired to head size 64 and stays as it is:
//   out[r][h] = softmax(scale * q[r][h] . K[row(r, s)][s, h]) V[row(r, s)][s, h]   for one new token per hypothesis.
// One wavefront per (row, head).  lane = (g, c): c = lane % (DH / 8) owns one 16-byte chunk of the head row, g = lane / (DH / 8) one of
// the 64 * 8 / DH key rows of a pass -- 4 rows of 256 bytes at head size 128, 2 rows of 512 bytes at 256 --, so every load instruction of the
// wave reads whole head rows and all passes of a batch are independent.  The key and value rows of UNR passes are requested together and
// folded into a running (max, sum, output) triple in f32: an online softmax.  One entry point carries the union of what the three 64-wide
// entry points take: q in place in a fused q | k | v row, a cache row table, a device `last_pos`, the fused append of this step's K / V,
// kv_div query rows per K / V row, a key mask.
#include <stdlib.h>
#include "common.h"

namespace {

struct WideAttP { const bf16_t* q; const bf16_t* k; const bf16_t* v; const unsigned char* mask; bf16_t* out; int R, S, H, kv_div; float scale;
                  const int* rowmap;              // optional [R][S]: cache row that holds position s of hypothesis r
                  const long long* last_pos;      // optional device scalar: only positions <= *last_pos exist (neither read nor attended)
                  const bf16_t* knew; const bf16_t* vnew; long ldq; };   // optional: this step's K / V rows [R][ldq]; attended to as position
                                                  // *last_pos and appended to row r of the caches

template <int DH>
__global__ __launch_bounds__(256) void decode_attn_wide_kernel(const WideAttP p) {
  constexpr int CH = DH / 8;           // 16-byte chunks of a head row = lanes per key row
  constexpr int G = 64 / CH;           // key rows per pass
  constexpr int UNR = 8;               // passes in flight
  __shared__ int sr[4][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + wv;
  if (w >= p.R * p.H) return;
  int r, h;
  if (p.kv_div > 1 && (p.kv_div & 3) == 0) {
    // hypotheses that share a K / V row: the four waves of a workgroup take four of them for ONE head and request the same lines at the
    // same time (see decode_attn_kernel)
    const int grp = blockIdx.x;
    h = grp % p.H;
    r = (grp / p.H) * 4 + wv;
  } else {
    r = w / p.H; h = w - r * p.H;
  }
  const int g = lane / CH, c = lane % CH;
  const long HD = (long)p.H * DH;
  float qr[8];
  {
    const uint4 u = *reinterpret_cast<const uint4*>(p.q + (long)r * (p.ldq ? p.ldq : HD) + h * DH + c * 8);
    qr[0] = lo_bf(u.x); qr[1] = hi_bf(u.x); qr[2] = lo_bf(u.y); qr[3] = hi_bf(u.y);
    qr[4] = lo_bf(u.z); qr[5] = hi_bf(u.z); qr[6] = lo_bf(u.w); qr[7] = hi_bf(u.w);
  }
  const long rk = r / p.kv_div;
  const bf16_t* kb = p.k + h * DH + c * 8;
  const bf16_t* vb = p.v + h * DH + c * 8;
  const unsigned char* mk = p.mask ? p.mask + rk * p.S : nullptr;
  const int Seff = p.last_pos ? max(0, min(p.S, (int)*p.last_pos + 1)) : p.S;
  const int passes = (Seff + G - 1) / G;
  const int snew = (p.knew && Seff > 0) ? Seff - 1 : -1;
  const bf16_t* kn = p.knew ? p.knew + (long)r * p.ldq + h * DH + c * 8 : nullptr;
  const bf16_t* vn = p.knew ? p.vnew + (long)r * p.ldq + h * DH + c * 8 : nullptr;
  if (snew >= 0 && g == 0) {
    const long dst = ((long)r * p.S + snew) * HD + h * DH + c * 8;
    *reinterpret_cast<uint4*>(const_cast<bf16_t*>(p.k) + dst) = *reinterpret_cast<const uint4*>(kn);
    *reinterpret_cast<uint4*>(const_cast<bf16_t*>(p.v) + dst) = *reinterpret_cast<const uint4*>(vn);
  }
  for (int s = lane; s < Seff; s += 64) sr[wv][s] = p.rowmap ? p.rowmap[(long)r * p.S + s] : (int)rk;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float mrun = -INFINITY, lrun = 0.f;               // running max (wave-uniform) and this key group's share of the running sum
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int it0 = 0; it0 < passes; it0 += UNR) {
    uint4 ku[UNR], vu[UNR];
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int s = (it0 + j) * G + g;
      const bool ok = s < Seff;
      const long off = ok ? ((long)sr[wv][s] * p.S + s) * HD : 0;
      ku[j] = ok ? *reinterpret_cast<const uint4*>(s == snew ? kn : kb + off) : make_uint4(0, 0, 0, 0);
      vu[j] = ok ? *reinterpret_cast<const uint4*>(s == snew ? vn : vb + off) : make_uint4(0, 0, 0, 0);
    }
    float sc[UNR];
    float bmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const int s = (it0 + j) * G + g;
      const uint4 u = ku[j];
      float a = lo_bf(u.x) * qr[0] + hi_bf(u.x) * qr[1] + lo_bf(u.y) * qr[2] + hi_bf(u.y) * qr[3] + lo_bf(u.z) * qr[4] + hi_bf(u.z) * qr[5] +
                lo_bf(u.w) * qr[6] + hi_bf(u.w) * qr[7];
#pragma unroll
      for (int x = 1; x < CH; x <<= 1) a += __shfl_xor(a, x, 64);                 // the CH lanes of a key row
      sc[j] = (s < Seff && !(mk && !mk[s])) ? a * p.scale : -INFINITY;
      bmax = fmaxf(bmax, sc[j]);
    }
#pragma unroll
    for (int x = CH; x < 64; x <<= 1) bmax = fmaxf(bmax, __shfl_xor(bmax, x, 64));   // the G key rows of a pass
    const float mnew = fmaxf(mrun, bmax);
    const float resc = (mrun == -INFINITY) ? 0.f : __expf(mrun - mnew);           // (mnew == -inf only while every key so far is masked)
    lrun *= resc;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= resc;
#pragma unroll
    for (int j = 0; j < UNR; ++j) {
      const float e = (sc[j] == -INFINITY || mnew == -INFINITY) ? 0.f : __expf(sc[j] - mnew);
      lrun += e;
      const uint4 u = vu[j];
      o[0] += e * lo_bf(u.x); o[1] += e * hi_bf(u.x); o[2] += e * lo_bf(u.y); o[3] += e * hi_bf(u.y);
      o[4] += e * lo_bf(u.z); o[5] += e * hi_bf(u.z); o[6] += e * lo_bf(u.w); o[7] += e * hi_bf(u.w);
    }
    mrun = mnew;
  }
  // every lane of a key group added the same e to lrun; the groups hold disjoint keys
#pragma unroll
  for (int x = CH; x < 64; x <<= 1) {
    lrun += __shfl_xor(lrun, x, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += __shfl_xor(o[j], x, 64);
  }
  const float inv = lrun > 0.f ? 1.f / lrun : 0.f;
  if (g == 0) {
    *reinterpret_cast<uint4*>(p.out + (long)r * HD + h * DH + c * 8) =
        make_uint4(pack2bf(o[0] * inv, o[1] * inv), pack2bf(o[2] * inv, o[3] * inv), pack2bf(o[4] * inv, o[5] * inv), pack2bf(o[6] * inv, o[7] * inv));
  }
}

}  // namespace

extern "C" {

int evk_decode_attention_wide(const void* q, int64_t ldq, void* k, void* v, const void* knew, const void* vnew, const unsigned char* mask,
                              const int32_t* rowmap, const int64_t* last_pos, void* out, int32_t R, int32_t S, int32_t heads, int32_t head_dim,
                              int32_t kv_div, float scale, evk_stream_t stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  EVK_REQUIRE(head_dim == 128 || head_dim == 256, "decode_attention_wide: head_dim must be 128 or 256 (got %d; 64 has its own entry points)", head_dim);
  EVK_REQUIRE(q && k && v && out && R > 0 && S > 0 && S <= 256 && heads > 0, "decode_attention_wide: null/empty, or S > 256");
  const int64_t HD = (int64_t)heads * head_dim;
  EVK_REQUIRE(kv_div >= 1 && R % kv_div == 0 && (int64_t)R * heads < INT32_MAX, "decode_attention_wide: R=%d must be a multiple of kv_div=%d", R, kv_div);
  EVK_REQUIRE(ldq == 0 || (ldq >= HD && ldq % 8 == 0), "decode_attention_wide: ldq=%lld must be a multiple of 8 and hold a row", (long long)ldq);
  EVK_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out) |
                reinterpret_cast<uintptr_t>(knew) | reinterpret_cast<uintptr_t>(vnew)) & 15) == 0, "decode_attention_wide: operands must be 16-byte aligned");
  EVK_REQUIRE((knew == nullptr) == (vnew == nullptr), "decode_attention_wide: the new key and value come as a pair");
  EVK_REQUIRE(!knew || (last_pos && kv_div == 1 && ldq > 0), "decode_attention_wide: the fused append needs last_pos, kv_div 1 and the rows' leading dimension");
  EVK_REQUIRE(!rowmap || kv_div == 1, "decode_attention_wide: a row table names one cache row per query row (kv_div 1)");
  WideAttP p{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, mask, (bf16_t*)out, R, S, heads, kv_div, scale, rowmap,
             reinterpret_cast<const long long*>(last_pos), (const bf16_t*)knew, (const bf16_t*)vnew, (long)ldq};
  ProfScope ps(EVK_FAM_NORM, s);
  const dim3 grid((int)cdiv((long)R * heads, 4));
  if (head_dim == 128) hipLaunchKernelGGL(decode_attn_wide_kernel<128>, grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL(decode_attn_wide_kernel<256>, grid, dim3(256), 0, s, p);
  return evk_check_launch("decode_attention_wide");
}

}  // extern "C"
