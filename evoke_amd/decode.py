"""Report generation on the HIP engine: beam search, and the sampling route (greedy / top-k / top-p) further down.

Semantics = AttModel._sample_beam (modules/att_model.py:98-137) + CaptionModel.beam_search / beam_step
(modules/caption_model.py:26-202, group_size = 1) + EncoderDecoder.core (modules/encoder_decoder.py:396-404).
The reference re-decodes the WHOLE prefix at every step (O(T^2) decoder work, O(T^2) Python-level relational-memory
steps) and walks a per-sample Python loop with .item() syncs; this engine is mathematically identical but
incremental: per-layer self-attention K/V caches, cross-attention K/V projected once, the relational memory carried
as state, the per-position conditional-LayerNorm inputs taken from the current memory, and all beam bookkeeping
(segmented top-k, EOS handling, the -1000 penalty, best-finished-beam tracking) done on the device.

Two tiers.  The SESSION (_Session and its subclasses, gpt2_decode._GPT2Session) keeps every buffer of a batch geometry on the decoder and
owns the one token-loop driver, _Session._drive: warm-up, capture of the per-token launch sequence, the replay plan, bursts -- or, with
_GRAPH_ENABLED off, the same launches issued eagerly.  Geometries its kernels do not serve (head dim other than 64, more than 256
positions) and EVK_DECODE_SESSION=0 take a plain HOST LOOP around _DecoderState.step(): _beam_eager and _sample_eager.
"""
import ctypes as C
import math
import os
import threading
import warnings
import weakref

import torch

from . import hip as H
from . import ops
from .config import tunable
from .ops import BF16, F32

# capture the per-token launch sequence in a HIP graph; False (read at every search): the session issues the same launches eagerly (debugging)
_GRAPH_ENABLED = [True]
_SESSION = [tunable('EVK_DECODE_SESSION', '1') != '0']           # the persistent session; off: the host loops (_beam_eager, _sample_eager)
_SPLIT_CLN = [tunable('EVK_DECODE_SPLIT_CLN', '1') != '0']       # first conditional-norm MLP layer as two launches (see cln_deltas)
# relational memory of the decode step in f32 (csrc/rm_f32.hip) -- the DEFAULT since round 4: the engine's log-probabilities stay within 5.3e-3 of
# the reference's at ALL 100 positions of the config-5 golden (the 16-bit recurrence: 2e-3 at position 10, 0.5 at position 90).  EVK_DECODE_RM_F32=0
# selects the 16-bit recurrence (evk_rm_decode_step), which drifts at depth and is kept for comparison only.
_RM_F32 = [os.environ.get('EVK_DECODE_RM_F32', '1') != '0']
# output projection + residual + the NEXT conditional layer norm, and the whole feed-forward + residual + next norm, as ONE launch each for 16
# hypotheses per workgroup (csrc/decode_rb.hip: weights streamed fragment-major from L2 into MFMA registers): 11 launches per decoder layer -> 6
_ROWBLOCK = [tunable('EVK_DECODE_ROWBLOCK', '1') != '0']
_RM_STEP = [tunable('EVK_DECODE_RM_STEP', '1') != '0']          # relational-memory step as one native call (evk_rm_decode_step)
_REPLAYER = [tunable('EVK_DECODE_REPLAYER', '1') != '0']      # re-issue the captured step with csrc/replay.hip instead of hipGraphLaunch
stats = {}                       # facts about the last beam_search call (bench.py reads the per-token step time from here)
_PLANS = []                      # (plan, graph, event recorded after the last replay): destroyed once the GPU has passed the event


_cap_streams = {}


def _capture_stream(dev, kind):
    key = (torch.device(dev).index, kind)
    st = _cap_streams.get(key)
    if st is None:
        st = _cap_streams[key] = torch.cuda.Stream(device=dev)
    return st


_plans_lock = threading.Lock()    # (searches driven by host threads end at the same time)


def _reap_plans(force=False):
    with _plans_lock:
        retired, _PLANS[:] = list(_PLANS), []
    keep = []
    for plan, graph, ev in retired:
        if force or ev.query():
            if force:
                ev.synchronize()
            H.lib.evk_replay_destroy(plan)
        else:
            keep.append((plan, graph, ev))
    with _plans_lock:
        _PLANS.extend(keep)


def _topk(x, k):
    rows, n = x.shape
    vals = torch.empty(rows, k, dtype=F32, device=x.device)
    idx = torch.empty(rows, k, dtype=torch.long, device=x.device)
    H.check(H.lib.evk_topk_rows(H.ptr(x), H.ptr(vals), H.ptr(idx), rows, n, k, H.stream()), 'topk_rows')
    return vals, idx


def _attend1(q, k, v, heads, mask):
    """One-query attention: q (R, 1, H*dh); k / v (R/div, S, H*dh) and mask uint8 (R/div, S) or None, where `div` consecutive
    query rows (the beams of one sample) share a K / V row -> (R, 1, H*dh)."""
    R = q.shape[0]
    Rk, S, HD = k.shape
    dh = HD // heads
    div = R // Rk
    if dh != 64 or S > 256:
        if div > 1:
            k, v = k.repeat_interleave(div, 0), v.repeat_interleave(div, 0)
            mask = mask.repeat_interleave(div, 0) if mask is not None else None
        return ops.attention(q, k, v, heads, mask=mask)
    out = torch.empty_like(q)
    H.check(H.lib.evk_decode_attention(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask) if mask is not None else None, H.ptr(out), R, S, heads,
                                       dh, div, C.c_float(1.0 / math.sqrt(dh)), H.stream()), 'decode_attention')
    return out


class _FusedDecodeWeights:
    """Inference-time weight packing for the per-token step (built once per generate call from the frozen parameters):
      * the 18 first-layer matrices of the nine ConditionalLayerNorm MLPs (mlp_gamma / mlp_beta, encoder_decoder.py:144-179)
        all read the same relational-memory row, so they become ONE GEMM with N = 18 x 512; their second layers run as ONE
        batched GEMM (batch 18), with the second-layer biases folded into per-norm effective gamma / beta vectors;
      * the self-attention q / k / v projections of each layer become one GEMM with N = 3 x 512.
    36 + 9 skinny launches per token turn into 2 + 3."""

    def __init__(self, model):
        dec = model.decoder
        self.clns = [layer.sublayer[j].norm for layer in dec.layers for j in range(3)]
        d = model.d_model
        w1, b1, w2, geff, beff = [], [], [], [], []
        for c in self.clns:
            for mlp, base in ((c.mlp_gamma, c.gamma), (c.mlp_beta, c.beta)):
                w1.append(mlp[0].weight.detach())
                b1.append(mlp[0].bias.detach())
                w2.append(mlp[2].weight.detach())
                (geff if mlp is c.mlp_gamma else beff).append((base.detach() + mlp[2].bias.detach()).float().contiguous())
        self.n = len(w1)
        self.d = d
        self.w1 = torch.cat(w1, 0).to(BF16).contiguous()                 # (18 d, slots*d)
        self.b1 = torch.cat(b1, 0).float().contiguous()
        self.w2 = torch.stack(w2, 0).to(BF16).contiguous()               # (18, d, d)
        self.geff, self.beff = geff, beff
        self.qkv_w = [torch.cat([l.self_attn.linears[i].weight.detach() for i in range(3)], 0).to(BF16).contiguous() for l in dec.layers]
        self.qkv_b = [torch.cat([l.self_attn.linears[i].bias.detach() for i in range(3)], 0).float().contiguous() for l in dec.layers]
        # row-block kernels (csrc/decode_rb.hip): fragment-major copies of the four 512 x 512 matrices of a layer that sit behind a residual
        self.rb = None
        if _ROWBLOCK[0] and d == 512 and all(tuple(l.feed_forward.w_1.weight.shape) == (512, 512) and tuple(l.feed_forward.w_2.weight.shape) == (512, 512)
                                             for l in dec.layers):
            def pack(w):
                out = torch.empty(512 * 512, dtype=BF16, device=w.device)
                H.check(H.lib.evk_decode_rb_pack(H.ptr(w.detach().to(BF16).contiguous()), H.ptr(out), H.stream()), 'decode_rb_pack')
                return out
            f32c = lambda b_: b_.detach().float().contiguous()          # noqa: E731
            self.rb = [dict(so=pack(l.self_attn.linears[3].weight), so_b=f32c(l.self_attn.linears[3].bias),
                            co=pack(l.src_attn.linears[3].weight), co_b=f32c(l.src_attn.linears[3].bias),
                            w1=pack(l.feed_forward.w_1.weight), b1=f32c(l.feed_forward.w_1.bias),
                            w2=pack(l.feed_forward.w_2.weight), b2=f32c(l.feed_forward.w_2.bias)) for l in dec.layers]
            fn = dec.norm
            self.final_g, self.final_b, self.final_eps = f32c(fn.gamma), f32c(fn.beta), float(fn.eps)
        # relational memory: the three projections of the token embedding (keys, values, gates) as one product, q | k | v of the memory as one
        rm = model.rm
        lin = rm.attn.linears
        self.rm_wx = torch.cat([lin[1].weight.detach(), lin[2].weight.detach(), rm.W.weight.detach()], 0).to(BF16).contiguous()      # (2048, 512)
        self.rm_bx = torch.cat([lin[1].bias.detach(), lin[2].bias.detach(), rm.W.bias.detach()], 0).float().contiguous()
        self.rm_wqkv = torch.cat([lin[i].weight.detach() for i in range(3)], 0).to(BF16).contiguous()                                 # (1536, 512)
        self.rm_bqkv = torch.cat([lin[i].bias.detach() for i in range(3)], 0).float().contiguous()
        self.rm_rest = [(m.weight.detach().to(BF16).contiguous(), m.bias.detach().float().contiguous()) for m in (lin[3], rm.mlp[0], rm.mlp[2], rm.U)]
        # ... and the f32 masters in the same stacking for the f32 recurrence (evk_rm_decode_step_f32)
        self.rm32_wx = torch.cat([lin[1].weight.detach(), lin[2].weight.detach(), rm.W.weight.detach()], 0).float().contiguous()
        self.rm32_wqkv = torch.cat([lin[i].weight.detach() for i in range(3)], 0).float().contiguous()
        self.rm32_rest = [m.weight.detach().float().contiguous() for m in (lin[3], rm.mlp[0], rm.mlp[2], rm.U)]

    def cln_deltas(self, memory):
        """memory (R, 1, slots*d) -> (18, R, d) bf16: [2i] = delta gamma, [2i+1] = delta beta of conditional norm i (bias folded out)."""
        R, K = memory.shape[0], memory.shape[-1]
        n, d = self.n, self.d
        hid = torch.empty(R, n * d, dtype=BF16, device=memory.device)
        # two column halves: 72 output tiles each, which the launcher gives to the latency-oriented skinny kernel (whole 256-deep K chunks
        # in flight, 128 x 32 tiles on 576 workgroups) instead of 144 tiles of the throughput kernel on 144 of 256 CUs (54 -> ~40 us)
        half = (n // 2) * d if _SPLIT_CLN[0] and n % 2 == 0 else n * d
        for off in range(0, n * d, half):
            ops.gemm(memory, self.w1[off:off + half], hid[:, off:], R, half, K, lda=K, ldb=K, ldc=n * d, bias=self.b1[off:off + half], act=H.ACT_RELU)
        out = torch.empty(n, R, d, dtype=BF16, device=memory.device)
        ops.gemm(hid, self.w2, out, R, d, d, lda=n * d, ldb=d, ldc=d, batch=(1, n), sA=(0, d), sB=(0, d * d), sC=(0, R * d))
        return out

    def norm(self, i, x, deltas):
        c = self.clns[i]
        return ops.layernorm(x, self.geff[i], self.beff[i], eps=c.eps, mode=1, dgam=deltas[2 * i].unsqueeze(1), dbet=deltas[2 * i + 1].unsqueeze(1))

    def rowblock(self, a, x, w2, b2, norm_i, deltas, w1=None, b1=None, sync=None):
        """(x + g . w2^T + b2, its next norm) with g = a or relu(a . w1^T + b1); norm_i = index of the conditional norm that follows, or None for
        the decoder's final norm.  One launch (evk_decode_rowblock)."""
        R = x.shape[0]
        y, n = torch.empty_like(x), torch.empty_like(x)
        if norm_i is None:
            g, b, eps, dg, db = self.final_g, self.final_b, self.final_eps, None, None
        else:
            c = self.clns[norm_i]
            g, b, eps, dg, db = self.geff[norm_i], self.beff[norm_i], float(c.eps), deltas[2 * norm_i], deltas[2 * norm_i + 1]
        H.check(H.lib.evk_decode_rowblock(H.ptr(a), H.ptr(w1) if w1 is not None else None, H.ptr(b1) if b1 is not None else None, H.ptr(w2), H.ptr(b2),
                                          H.ptr(x), H.ptr(y), H.ptr(g), H.ptr(b), H.ptr(dg) if dg is not None else None,
                                          H.ptr(db) if db is not None else None, dg.stride(0) if dg is not None else 0, C.c_float(eps), H.ptr(n), R,
                                          H.ptr(sync) if sync is not None else None, H.stream()), 'decode_rowblock')
        return y, n

    def qkv(self, li, n):
        R, d = n.shape[0], self.d
        out = torch.empty(R, 3 * d, dtype=BF16, device=n.device)
        ops.gemm(n, self.qkv_w[li], out, R, 3 * d, d, lda=d, ldb=d, ldc=3 * d, bias=self.qkv_b[li])
        return out


def _fused_weights(model):
    """_FusedDecodeWeights of `model`, rebuilt only when a parameter of the decoder changed (torch version counters + the optimizer's
    weight epoch: ops.WEIGHT_EPOCH) -- 28 MB of concatenations per generate call otherwise"""
    ps = [p for p in model.decoder.parameters()]
    key = (ops.WEIGHT_EPOCH[0], tuple(p._version for p in ps), ps[0].device, ps[0].data_ptr())
    hit = getattr(model, '_evk_fused_decode', None)
    if hit is None or hit[0] != key:
        hit = (key, _FusedDecodeWeights(model))
        model._evk_fused_decode = hit
    return hit[1]


class _DecoderState:
    """Incremental state of R = batch*beam hypotheses."""

    def __init__(self, dec, enc, src_mask, max_len, cross_kv=None, rows=None, row_table=False):
        """cross_kv: ([K per layer], [V per layer]) already projected from `enc` (the session computes them once for both the first,
        B-row step and the R-row steps); rows: hypothesis count of the self-attention caches / memory (default: enc rows); row_table:
        build the cache row table that step_static needs (a session's R-row state; head dim 64, max_len <= 256)."""
        model = dec.model
        self.dec, self.model = dec, model
        R, d = (enc.shape[0] if rows is None else rows), model.d_model
        self.enc, self.src_mask = enc, src_mask
        self.mem = model.rm.init_memory(R, enc.device)
        self.t = 0
        # cache row table of step_static: position s of hypothesis r lives in cache row anc[r, s], so that a beam search re-orders
        # this table (100 KB) and not the self-attention caches (6 x 26 MB gathered and copied)
        self.anc = self.rows = None
        if row_table:
            self.rows = torch.arange(R, dtype=torch.int32, device=enc.device).view(R, 1)
            self.anc = self.rows.expand(R, max_len).contiguous()
        self.logit_scale = 1.0           # 1 / temperature of the beam search's later steps (step_static only; caption_model.py:196)
        # cross-attention map history f32 [positions][R][n_layers * S] of a search that returns its maps (set by the session), or None: the
        # step then writes, from the cross-attention launch itself, layer i's head-mean probabilities of every row into columns
        # [i * S, (i + 1) * S) of the slab of the position it computes (evk_decode_attention_maps)
        self.maps = None
        self.tmem = None                 # tanh(memory), kept beside the memory by the session path (evk_rm_decode_step)
        # the f32 relational memory (evk_rm_decode_step_f32): the state, the unrounded token embedding, scratch, the 16-bit row for the decoder
        self.mem32 = self.emb32 = self.rm32_ws = self.rm32_out = None
        if _RM_F32[0]:
            self.mem32 = self.mem.float().contiguous()
            self.emb32 = torch.empty(R, d, dtype=F32, device=enc.device)
            self.rm32_ws = torch.empty(H.lib.evk_rm_decode_f32_ws_bytes(R), dtype=torch.uint8, device=enc.device)
            self.rm32_out = torch.empty(R, 1, self.mem[0].numel(), dtype=BF16, device=enc.device)
        self.fused = _fused_weights(model)
        self.kc, self.vc, self.ks, self.vs = [], [], [], []
        for i, layer in enumerate(model.decoder.layers):
            self.kc.append(layer.src_attn.linears[1](enc) if cross_kv is None else cross_kv[0][i])
            self.vc.append(layer.src_attn.linears[2](enc) if cross_kv is None else cross_kv[1][i])
            self.ks.append(torch.zeros(R, max_len, d, dtype=BF16, device=enc.device))
            self.vs.append(torch.zeros(R, max_len, d, dtype=BF16, device=enc.device))

    def rm_step_f32(self):
        """one token of the relational memory in f32: self.emb32 (filled by the embedding launch) and self.mem32 -> self.mem32 (in place),
        returns the 16-bit memory row (R, 1, 1536) for the conditional layer norms"""
        fw = self.fused
        (_, bo), (_, b0), (_, b2), (_, bu) = fw.rm_rest
        wo, w0, w2, wu = fw.rm32_rest
        Rh = self.emb32.shape[0]
        H.check(H.lib.evk_rm_decode_step_f32(H.ptr(self.emb32), H.ptr(fw.rm32_wx), H.ptr(fw.rm_bx), H.ptr(self.mem32), H.ptr(fw.rm32_wqkv), H.ptr(fw.rm_bqkv),
                                             H.ptr(wo), H.ptr(bo), H.ptr(w0), H.ptr(b0), H.ptr(w2), H.ptr(b2), H.ptr(wu), H.ptr(bu), H.ptr(self.rm32_out),
                                             H.ptr(self.rm32_ws), self.rm32_ws.numel(), Rh, H.stream()), 'rm_decode_step_f32')
        return self.rm32_out

    def expand_cross(self, n):
        """n hypotheses per sample for the host-position step(), whose attention wants one K / V row per query row (step_static reads
        one row per SAMPLE instead: evk_decode_attention kv_div)"""
        self.kc = [k.repeat_interleave(n, 0) for k in self.kc]
        self.vc = [v.repeat_interleave(n, 0) for v in self.vc]
        self.src_mask = self.src_mask.repeat_interleave(n, 0) if self.src_mask is not None else None

    def reorder(self, ix):
        """first beam expansion (B -> B*beam hypotheses).  The encoder states, their mask and the cross-attention K/V stay at
        one row per SAMPLE: every beam of a sample reads the same row (evk_decode_attention kv_div; step() needs expand_cross)."""
        self.mem = self.mem.index_select(0, ix)
        if self.mem32 is not None:
            self.mem32 = self.mem32.index_select(0, ix)
            n = ix.numel()
            if self.emb32.shape[0] != n:
                self.emb32 = torch.empty(n, self.emb32.shape[1], dtype=F32, device=ix.device)
                self.rm32_ws = torch.empty(H.lib.evk_rm_decode_f32_ws_bytes(n), dtype=torch.uint8, device=ix.device)
                self.rm32_out = torch.empty(n, 1, self.mem[0].numel(), dtype=BF16, device=ix.device)
        t = self.t
        for i in range(len(self.ks)):
            if ix.numel() != self.ks[i].shape[0]:
                nk = torch.zeros(ix.numel(), *self.ks[i].shape[1:], dtype=BF16, device=ix.device)
                nv = torch.zeros_like(nk)
                nk[:, :t] = self.ks[i][:, :t].index_select(0, ix)
                nv[:, :t] = self.vs[i][:, :t].index_select(0, ix)
                self.ks[i], self.vs[i] = nk, nv
            else:
                self.ks[i][:, :t] = self.ks[i][:, :t].index_select(0, ix)
                self.vs[i][:, :t] = self.vs[i][:, :t].index_select(0, ix)

    def _self_attend(self, i, qkv, pos):
        """self-attention of layer i over the row table: q read in place from qkv (R, q | k | v), this step's K / V attended to straight
        from qkv and appended to the caches at position *pos by the same kernel -> (R, 1, d)"""
        d = self.model.d_model
        h = self.model.decoder.layers[0].self_attn.h
        c = torch.empty(qkv.shape[0], 1, d, dtype=qkv.dtype, device=qkv.device)
        H.check(H.lib.evk_decode_attention_qkv(H.ptr(qkv), qkv.stride(0), H.ptr(self.ks[i]), H.ptr(self.vs[i]), H.ptr(self.anc), H.ptr(pos),
                                               H.ptr(c), qkv.shape[0], self.ks[i].shape[1], h, d // h, C.c_float(1.0 / math.sqrt(d // h)),
                                               H.stream()), 'decode_attention_qkv')
        return c

    def _cross_attend(self, i, q, pos=None):
        """cross-attention of layer i for the queries q (R, 1, d) -> (R, 1, d).  With a map history (self.maps) the same launch also writes
        the rows' head-mean probabilities into the slab of position *pos (a device scalar; None: slab 0)."""
        h = self.model.decoder.layers[0].self_attn.h
        if self.maps is None:
            return _attend1(q, self.kc[i], self.vc[i], h, self.src_mask)
        R = q.shape[0]
        Rk, S, HD = self.kc[i].shape
        out = torch.empty_like(q)
        H.check(H.lib.evk_decode_attention_maps(H.ptr(q), H.ptr(self.kc[i]), H.ptr(self.vc[i]), H.ptr(self.src_mask), H.ptr(out),
                                                self.maps.data_ptr() + 4 * i * S, self.maps.shape[-1], H.ptr(pos), self.maps.stride(0), R, S, h,
                                                HD // h, R // Rk, C.c_float(1.0 / math.sqrt(HD // h)), H.stream()), 'decode_attention_maps')
        return out

    def step_static(self, it, pos, out=None, seed_rows=True):
        """step() with the position held in a device tensor `pos` (1,) and self-attention over the cache row table (positions <= *pos,
        read from the device): no host-side shape depends on the step index, so the launch sequence can be captured once in a HIP graph
        and replayed.  Needs a state built with row_table=True."""
        model = self.model
        if seed_rows:
            self.anc.index_copy_(1, pos, self.rows)      # this step's K / V are written to the hypothesis's own cache row
        # the positional row is picked on the device (pos is a device scalar inside the captured step)
        emb = ops.embedding(it.view(-1, 1).contiguous(), model.tgt_embed[0].lut.weight, pos=model.tgt_embed[1].pe[0], scale=math.sqrt(model.d_model),
                            pos0=pos, out32=self.emb32)
        fw, d = self.fused, model.d_model
        if self.mem32 is not None:
            memory = self.rm_step_f32()
        elif self.tmem is not None and _RM_STEP[0]:
            # the whole relational-memory step in one native call: 8 launches, memory and tanh(memory) updated in place
            Rh = emb.shape[0]
            if getattr(self, 'rm_ws', None) is None:
                self.rm_ws = torch.empty(H.lib.evk_rm_decode_ws_bytes(Rh), dtype=torch.uint8, device=emb.device)
                self.rm_out = torch.empty(Rh, 1, self.mem[0].numel(), dtype=BF16, device=emb.device)
            (wo, bo), (w0, b0), (w2, b2), (wu, bu) = fw.rm_rest
            H.check(H.lib.evk_rm_decode_step(H.ptr(emb), H.ptr(fw.rm_wx), H.ptr(fw.rm_bx), H.ptr(self.mem), H.ptr(self.tmem), H.ptr(fw.rm_wqkv),
                                             H.ptr(fw.rm_bqkv), H.ptr(wo), H.ptr(bo), H.ptr(w0), H.ptr(b0), H.ptr(w2), H.ptr(b2), H.ptr(wu), H.ptr(bu),
                                             H.ptr(self.rm_out), H.ptr(self.rm_ws), self.rm_ws.numel(), Rh, H.stream()), 'rm_decode_step')
            memory = self.rm_out
        else:
            memory, new_mem = model.rm.run(emb, self.mem)
            ops.copy_kernel(self.mem, new_mem)
        deltas = fw.cln_deltas(memory)
        x = emb.view(-1, d)
        rb = fw.rb if x.is_contiguous() else None
        if rb is not None:
            # row-block path: 6 launches per layer -- q|k|v, self-attention, [o-proj + residual + norm], q, cross-attention, [o-proj + residual +
            # norm], [feed-forward + residual + next norm]
            nl = len(model.decoder.layers)
            if getattr(self, 'rb_sync', None) is None:
                # exchange buffer of the split row blocks: zeroed once, owned by this state (= this search's launch sequence)
                self.rb_sync = torch.zeros(H.lib.evk_decode_rowblock_sync_bytes(x.shape[0]), dtype=torch.uint8, device=x.device)
            n = fw.norm(0, x, deltas).view(-1, d)
            for i, layer in enumerate(model.decoder.layers):
                w = rb[i]
                c = self._self_attend(i, fw.qkv(i, n), pos)
                x, n = fw.rowblock(c.view(-1, d), x, w['so'], w['so_b'], 3 * i + 1, deltas, sync=self.rb_sync)
                q = layer.src_attn.linears[0](n)
                c = self._cross_attend(i, q.view(-1, 1, d), pos)
                x, n = fw.rowblock(c.view(-1, d), x, w['co'], w['co_b'], 3 * i + 2, deltas, sync=self.rb_sync)
                x, n = fw.rowblock(n, x, w['w2'], w['b2'], 3 * (i + 1) if i + 1 < nl else None, deltas, w1=w['w1'], b1=w['b1'], sync=self.rb_sync)
        else:
            # one launch per projection, norm and attention (the only route for d_model or d_ff other than 512)
            for i, layer in enumerate(model.decoder.layers):
                c = self._self_attend(i, fw.qkv(i, fw.norm(3 * i, x, deltas).view(-1, d)), pos)
                x = layer.self_attn.linears[3](c.view(-1, d), resid=x)
                ca = layer.src_attn
                q = ca.linears[0](fw.norm(3 * i + 1, x, deltas))
                c = self._cross_attend(i, q.view(-1, 1, d), pos)
                x = ca.linears[3](c.view(-1, d), resid=x)
                x = layer.feed_forward(fw.norm(3 * i + 2, x, deltas), resid=x)
            n = model.decoder.norm(x).view(-1, d)
        # the logits go straight into a persistent f32 buffer whose pad columns were zeroed once (no per-step fill)
        lg = self.dec.logit
        V1 = lg.weight.shape[0]
        Np = (V1 + 7) // 8 * 8
        if getattr(self, 'logits_buf', None) is None or self.logits_buf.shape[0] != x.shape[0]:
            self.logits_buf = torch.zeros(x.shape[0], Np, dtype=F32, device=x.device)
        ops.gemm(n, ops.shadow(lg.weight, pad_rows=(V1 != Np)), self.logits_buf, x.shape[0], V1, d, lda=d, ldb=d, ldc=Np, bias=lg.bias)
        return ops.log_softmax(self.logits_buf, self.dec.vocab_size + 1, out=out, scale=self.logit_scale)

    def step(self, it):
        """it (R,) token ids at position self.t -> f32 log-probs (R, V+1) of the next token."""
        model, t = self.model, self.t
        h = model.decoder.layers[0].self_attn.h
        pe = model.tgt_embed[1].pe[0][t:t + 1]
        emb = ops.embedding(it.view(-1, 1).contiguous(), model.tgt_embed[0].lut.weight, pos=pe, scale=math.sqrt(model.d_model), out32=self.emb32)
        if self.mem32 is not None:
            memory = self.rm_step_f32().clone()
        else:
            memory, self.mem = model.rm.run(emb, self.mem)          # (R, 1, slots*d), carried memory
        x = emb
        for i, layer in enumerate(model.decoder.layers):
            n = layer.sublayer[0].norm(x, memory)
            sa = layer.self_attn
            q = sa.linears[0](n)
            self.ks[i][:, t:t + 1] = sa.linears[1](n)
            self.vs[i][:, t:t + 1] = sa.linears[2](n)
            c = ops.attention(q, self.ks[i][:, :t + 1].contiguous(), self.vs[i][:, :t + 1].contiguous(), h)
            x = sa.linears[3](c, resid=x)
            n = layer.sublayer[1].norm(x, memory)
            ca = layer.src_attn
            if self.maps is None:
                c = ops.attention(ca.linears[0](n), self.kc[i], self.vc[i], h, mask=self.src_mask)
            else:
                c = self._cross_attend(i, ca.linears[0](n).contiguous())      # (a one-position state: slab 0)
            x = ca.linears[3](c, resid=x)
            n = layer.sublayer[2].norm(x, memory)
            x = layer.feed_forward(n, resid=x)
        out = model.decoder.norm(x)
        logits = self.dec.logit(out, out_f32=True)
        self.t = t + 1
        return ops.log_softmax(logits.view(logits.shape[0], -1), self.dec.vocab_size + 1)


class _Session:
    """What a decode session over B samples x R rows x max_len positions owns on the device whatever the search -- self-attention caches,
    cache row table, cross-attention K / V, relational memory, the log-probability buffer, the position counter -- allocated ONCE and kept
    on the decoder, together with the captured per-token launch sequence and its replay plan.  A generate call then only refills the
    buffers (cross K / V of the new batch, the first position's state) and replays: no allocation, no capture, no plan build per batch
    (13 ms of host time per 64-study batch otherwise, during which the decode stream sits idle).  A subclass supplies _body() (the
    launches of one token step) and _run_iter() (what happens around the token loop)."""

    def _init_driving(self, dec, slot):
        """what _drive, run_iter and __del__ read whatever the backend: every subclass calls this, also one that allocates buffers of its own
        (gpt2_decode._GPT2Session).  Beyond these, _drive needs words, ticket, pos and logp_buf on the device."""
        self.dec, self.slot = dec, slot
        self.graph = self.plan = None     # the captured per-token step and its replay plan
        self.issued = 0                   # bodies issued by the last _drive, warm-up included

    def __init__(self, dec, B, R, max_len, S, dev, slot=0):
        model = dec.model
        self._init_driving(dec, slot)
        d, nl = model.d_model, len(model.decoder.layers)
        self.B, self.max_len, self.R = B, max_len, R
        self.kc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.vc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.st = None                    # R-row decoder state, built on first use (needs an encoder output for its geometry)
        self.words = torch.empty(R, dtype=torch.long, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pos = torch.ones(1, dtype=torch.long, device=dev)
        self.logp_buf = torch.empty(R, dec.vocab_size + 1, dtype=F32, device=dev)
        self.fused_key = None
        # the encoder key mask of the CURRENT batch, in a buffer the session owns: the captured per-token step records a pointer, so a
        # later batch's mask must land at the same address (a session serves masked or unmasked batches, never both: part of its key)
        self.src_mask = None

    def __del__(self):
        if getattr(self, 'plan', None) is not None:
            try:
                torch.cuda.synchronize()
                H.lib.evk_replay_destroy(self.plan)
            except Exception:          # noqa: BLE001 -- interpreter shutdown
                pass

    def run(self, *args, **kw):
        it = self.run_iter(*args, **kw)
        try:
            while True:
                next(it)
        except StopIteration as e:
            return e.value

    def run_iter(self, *args, **kw):
        """_run_iter under eval mode and no_grad for as long as the generator RUNS (a generator's body executes at next(), long after
        the caller's own eval / no_grad scope has been left; no_grad is per THREAD: the scope is opened around every next(), whichever
        thread calls it)"""
        it = self._run_iter(*args, **kw)
        dec = self.dec
        while True:
            # (nn.Module.eval / train walk the whole module tree: only when the decoder really is in training mode -- the serving loop
            # has put the model in eval mode once and pays nothing here)
            was_training = dec.training
            if was_training:
                dec.eval()
            try:
                with torch.no_grad():
                    v = next(it)
            except StopIteration as e:
                return e.value
            finally:
                if was_training:
                    dec.train(True)
            yield v

    def _refill(self, enc, src_mask):
        """the new batch into the session's buffers (the captured step reads them there); (re)builds the R-row state when the decoder's
        derived weights changed -> the session's copy of the encoder key mask (or None)"""
        dec, B, dev = self.dec, self.B, enc.device
        model = dec.model
        # cross-attention K / V of this batch
        for i, layer in enumerate(model.decoder.layers):
            ops.copy_kernel(self.kc[i], layer.src_attn.linears[1](enc))
            ops.copy_kernel(self.vc[i], layer.src_attn.linears[2](enc))
        if src_mask is not None:
            if self.src_mask is None:
                self.src_mask = torch.empty(B, src_mask.shape[-1], dtype=torch.uint8, device=dev)
            if tuple(src_mask.shape) != tuple(self.src_mask.shape) or src_mask.dtype != torch.uint8:
                raise ValueError('decode session: encoder mask %s %s does not fit the session (%s uint8)'
                                 % (tuple(src_mask.shape), src_mask.dtype, tuple(self.src_mask.shape)))
            self.src_mask.copy_(src_mask)                 # (B x S bytes, not a multiple of 4 in general: torch's copy, outside the capture)
            src_mask = self.src_mask
        elif self.src_mask is not None:
            raise ValueError('decode session built for masked encoder states got an unmasked batch')
        fused = _fused_weights(model)
        if self.st is None or self.fused_key is not fused:
            # (re)build the R-row state around the session's buffers; derived weights changed -> the captured step is stale as well
            self.st = _DecoderState(dec, enc, src_mask, self.max_len, cross_kv=(self.kc, self.vc), rows=self.R, row_table=True)
            self.fused_key = fused
            self._retire_plan()
        self.st.enc, self.st.src_mask = enc, src_mask
        return src_mask

    def _retire_plan(self):
        """the captured step is stale (its weights changed): its plan is destroyed once the GPU has passed the replays issued so far"""
        if self.plan is not None:
            ev = torch.cuda.Event()
            ev.record()
            with _plans_lock:
                _PLANS.append((self.plan, self.graph, ev))
        self.graph = self.plan = None

    def _drive(self, n_body, first, step_hook, burst, extra=(), stop=None):
        """the token loop: n_body times _body(), body number i writing the log-probabilities of position i + first (step_hook(position,
        logp_buf, *extra) is called right after it).  On first use two bodies run as warm-up, the third is captured and turned into a
        replay plan; the loop then replays.  With _GRAPH_ENABLED off every body is issued eagerly instead: nothing is captured, and a
        captured step the session holds is kept but not replayed.  A generator: yields after every issued step (see _run_iter of the
        subclasses).
        stop(i) (optional, host only): asked before body number i (or the burst that starts with it) is issued; True ends the loop there."""
        dev = self.logp_buf.device
        done = 0
        cur = torch.cuda.current_stream()
        graph_on = _GRAPH_ENABLED[0]
        if self.graph is None and n_body > 3 and graph_on:
            hook = step_hook if step_hook is not None else (lambda *a: None)
            side = _capture_stream(dev, ('warm', self.slot))
            side.wait_stream(cur)
            with torch.cuda.stream(side):                           # warm-up iterations (real steps) off the launching stream
                self._body()
                hook(first, self.logp_buf, *extra)
                self._body()
                hook(first + 1, self.logp_buf, *extra)
            cur.wait_stream(side)
            done = 2
            try:
                # captured by hand (capture_begin / capture_end on a side stream), not through torch.cuda.graph(): the context manager
                # opens with a DEVICE-WIDE synchronize, which would make this decode wait for the next batch's encoders
                graph = torch.cuda.CUDAGraph(keep_graph=_REPLAYER[0])
                cap = _capture_stream(dev, ('capture', self.slot))
                cap.wait_stream(cur)
                with torch.cuda.stream(cap):
                    # (a pool of the session's own: searches in flight at the same time replay concurrently, and a handle must not
                    # outlive the last graph that used it)
                    self.pool = torch.cuda.graph_pool_handle()
                    # (thread_local: the worker threads of generate_pipelined download results / record events on OTHER streams meanwhile)
                    graph.capture_begin(pool=self.pool, capture_error_mode='thread_local')
                    try:
                        self._body()
                    finally:
                        graph.capture_end()
                cur.wait_stream(cap)
                self.graph = graph
            except Exception as e:                                   # stay on the HIP path, just without the graph
                warnings.warn('decode: HIP graph capture failed (%s); running the steps eagerly' % e)
                self.graph = None
            if self.graph is not None and _REPLAYER[0]:
                # the library's own replayer (csrc/replay.hip): plain launches, ~3 us of host time per node (hipGraphLaunch: 7-12 us)
                plan = H.lib.evk_replay_build(C.c_void_p(self.graph.raw_cuda_graph()), 16)
                if not plan:
                    warnings.warn('decode: replay plan refused (%s); using hipGraphLaunch' % H.lib.evk_last_error().decode())
                    if hasattr(self.graph, 'instantiate'):
                        self.graph.instantiate()
                self.plan = plan or None
                if self.plan is not None:
                    info = (C.c_int64 * 7)()
                    H.check(H.lib.evk_replay_info(self.plan, info), 'replay_info')
                    self.step_launches = int(info[1])                 # kernel nodes of ONE captured token step
        stats['step_launches'] = getattr(self, 'step_launches', None)
        graph, plan = (self.graph, self.plan) if graph_on else (None, None)
        bursts = burst > 0 and plan is not None and step_hook is None
        if bursts:
            yield -1
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        it_ = done
        while bursts and it_ < n_body:
            if stop is not None and stop(it_):
                n_body = it_
                break
            n = min(int(burst), n_body - it_)
            H.check(H.lib.evk_replay_run_n(plan, H.stream(), n), 'replay_run_n')
            it_ += n
            yield it_ - 1
        for it_ in range(it_, n_body):
            if stop is not None and stop(it_):
                n_body = it_
                break
            if plan is not None:
                H.check(H.lib.evk_replay_run(plan, H.stream()), 'replay_run')
            elif graph is not None:
                graph.replay()
            else:
                self._body()
            if step_hook is not None:
                step_hook(it_ + first, self.logp_buf, *extra)
            yield it_
        ev1.record()
        stats['step_events'] = (ev0, ev1, max(0, n_body - done))      # per-token step time = elapsed / count (bench.py)
        self.issued = max(n_body, done)                                  # bodies issued, warm-up included
        stats['graph'] = graph is not None
        stats['replayer'] = plan is not None
        stats['fused_bookkeeping'] = True


_warned = set()


def _length_divisors(length_penalty, max_len):
    """utils.penalty_builder (modules/utils.py:160-186) as a table: the modifier the running sum of a hypothesis of length t + 1 is divided
    by, in Python floats as the reference computes it -> list of max_len floats, or None for '' (identity).  'avg_<x>': the length;
    'wu_<a>': (5 + length)^a / 6^a.  Anything else is a ValueError (the reference returns None there and fails at the first finished beam)."""
    if length_penalty == '':
        return None
    parts = str(length_penalty).split('_')
    if len(parts) != 2 or parts[0] not in ('wu', 'avg'):
        raise ValueError("length_penalty must be '', 'avg_<x>' or 'wu_<alpha>', not %r" % (length_penalty,))
    try:
        alpha = float(parts[1])
    except ValueError:
        raise ValueError("length_penalty must be '', 'avg_<x>' or 'wu_<alpha>', not %r" % (length_penalty,)) from None
    if parts[0] == 'avg':
        return [float(t) for t in range(1, max_len + 1)]
    return [((5 + t) ** alpha) / ((5 + 1) ** alpha) for t in range(1, max_len + 1)]


def beam_options(args, beam, return_logprobs=False, return_attention=False):
    """The options of CaptionModel.beam_search / AttModel._sample_beam read from `args` and validated -> None when every one is at its
    default and neither log-probabilities nor attention maps are asked for (the search then runs exactly the launches it always ran), else a
    dict (part of the session key: the options are kernel arguments of the captured step).  `return_attention` is an entry of the dict only
    when set, so the keys of every other search stay what they were."""
    if args.get('group_size', 1) != 1:
        raise NotImplementedError("diverse beam search (group_size > 1) is not on the path: the reference's own grouped search fails "
                                  '(CaptionModel.beam_search calls self.repeat_tensor, which no class defines), so there is nothing to match')
    if args.get('suppress_UNK', 0) and 'suppress_UNK' not in _warned:
        _warned.add('suppress_UNK')
        warnings.warn("suppress_UNK is inert: the reference applies it only when the model has a `vocab` attribute, which EncoderDecoder "
                      'never has (caption_model.py:152); it has no effect here either')
    n = int(args.get('sample_n', 1))
    if n != 1 and n != beam:
        raise ValueError('beam search: sample_n must be 1 or beam_size (%d), not %d' % (beam, n))
    temperature = float(args.get('temperature', 1.0))
    if not (temperature > 0 and math.isfinite(temperature)):
        raise ValueError('temperature must be positive')
    length_penalty = args.get('length_penalty', '') or ''
    _length_divisors(length_penalty, 1)
    opts = dict(temperature=temperature, decoding_constraint=int(bool(args.get('decoding_constraint', 0))), length_penalty=str(length_penalty),
                sample_n=n, return_logprobs=bool(return_logprobs))
    if return_attention:
        opts['return_attention'] = True
    elif opts == dict(temperature=1.0, decoding_constraint=0, length_penalty='', sample_n=1, return_logprobs=False):
        return None
    return opts


class _BeamLists:
    """What evk_beam_step_opts keeps beside the plain bookkeeping: per study the sorted list of finished hypotheses (score f64, length,
    words, and per position the row whose log-probabilities scored it), the length-penalty table, and -- only when log-probabilities are
    asked for -- the history of every step's rows (max_len x R x (V+1) f32: ~225 MB at 32 studies x beam 4 x 100 positions x 4.4 k words)."""

    def __init__(self, dec, B, beam, max_len, dev, opts, S=0):
        self.dec, self.B, self.beam, self.max_len, self.opts = dec, B, beam, max_len, opts
        self.score = torch.empty(B, beam, dtype=torch.float64, device=dev)
        self.len = torch.empty(B, beam, dtype=torch.int32, device=dev)
        self.seq = torch.empty(B, beam, max_len, dtype=torch.long, device=dev)
        self.anc = torch.empty(B, beam, max_len, dtype=torch.int32, device=dev)
        div = _length_divisors(opts['length_penalty'], max_len)
        self.len_div = torch.tensor(div, dtype=torch.float64, device=dev) if div is not None else None
        self.hist = torch.empty(max_len, B * beam, dec.vocab_size + 1, dtype=F32, device=dev) if opts['return_logprobs'] else None
        # the cross-attention maps of every step's rows, indexed like hist (slab t = the step that computed position t, so `anc` names the
        # row): max_len x R x (n_layers * S) f32, 22 MB at 32 studies x beam 4 x 100 positions x 3 layers x 144 patch tokens
        self.nl = len(dec.model.decoder.layers)
        self.hist_attn = torch.zeros(max_len, B * beam, self.nl * S, dtype=F32, device=dev) if opts.get('return_attention') else None

    def reset(self):
        self.score.fill_(-float('inf'))
        self.len.zero_()
        self.seq.fill_(self.dec.pad_idx)
        self.anc.zero_()

    def result(self, return_scores):
        """-> seq (rows, max_len) [, seq_logprobs (rows, max_len, V+1) f32] [, attention (rows, max_len, n_layers, S) f32] [, scores (rows,)
        f64], rows = B * sample_n, the entries of a study next to each other in list order (att_model.py:126-135)"""
        n, B, max_len, V1 = self.opts['sample_n'], self.B, self.max_len, self.dec.vocab_size + 1
        out = [self.seq[:, :n].reshape(B * n, max_len).clone()]
        if self.hist is not None:
            slp = torch.empty(B * n, max_len, V1, dtype=F32, device=self.seq.device)
            H.check(H.lib.evk_beam_gather_logprobs(H.ptr(self.hist), H.ptr(self.anc), H.ptr(self.len), H.ptr(slp), B, self.beam, n, max_len, V1,
                                                   H.stream()), 'beam_gather_logprobs')
            out.append(slp)
        if self.hist_attn is not None:
            # the same gather with n_layers * S columns: row t of an entry comes from the row that scored its word t
            W = self.hist_attn.shape[-1]
            att = torch.empty(B * n, max_len, W, dtype=F32, device=self.seq.device)
            H.check(H.lib.evk_beam_gather_logprobs(H.ptr(self.hist_attn), H.ptr(self.anc), H.ptr(self.len), H.ptr(att), B, self.beam, n, max_len, W,
                                                   H.stream()), 'beam_gather_logprobs')
            out.append(att.view(B * n, max_len, self.nl, W // self.nl))
        if return_scores:
            out.append(self.score[:, :n].reshape(-1).clone())
        return out[0] if len(out) == 1 else tuple(out)


def _beam_step(dec, lp, beam, B, max_len, pos, last, beam_sum, beam_seq, best_p, best_seq, words, mem, mem_row, anc, pos_advance, ticket, mem2,
               lists=None):
    """one launch of csrc/beam.hip: evk_beam_step, or evk_beam_step_opts when the search carries options (`lists`)"""
    head = (H.ptr(lp), lp.shape[-1], dec.vocab_size + 1, beam, B, max_len, H.ptr(pos), dec.eos_idx, int(last), H.ptr(beam_sum), H.ptr(beam_seq),
            H.ptr(best_p), H.ptr(best_seq), H.ptr(words), H.ptr(mem), mem_row, H.ptr(anc), anc.shape[1] if anc is not None else 0,
            H.ptr(pos_advance), H.ptr(ticket), H.ptr(mem2))
    if lists is None:
        H.check(H.lib.evk_beam_step(*head, H.stream()), 'beam_step')
    else:
        H.check(H.lib.evk_beam_step_opts(*head, dec.pad_idx, lists.opts['decoding_constraint'], H.ptr(lists.len_div), H.ptr(lists.score),
                                         H.ptr(lists.len), H.ptr(lists.seq), H.ptr(lists.anc), H.ptr(lists.hist), H.stream()), 'beam_step_opts')


def _beam_first_position(dec, logp0, beam, B, max_len, beam_sum, beam_seq, best_p, best_seq, words, lists):
    """position 0 of a search with options through the same kernel, so that the finished list sees an [EOS] at position 0 and max_len == 1:
    the study's one row stands in for all `beam` source rows, of which only the first has a finite running sum (-inf + logp never wins)"""
    V1 = dec.vocab_size + 1
    beam_sum.fill_(-float('inf'))
    beam_sum[:, 0] = 0.0
    lp0 = logp0.view(B, -1)[:, :V1].repeat_interleave(beam, 0).contiguous()
    pos0 = torch.zeros(1, dtype=torch.long, device=lp0.device)
    _beam_step(dec, lp0, beam, B, max_len, pos0, max_len == 1, beam_sum, beam_seq, best_p, best_seq, words, None, 0, None, None, None, None, lists)


def _beam_book(dec, logp, t, base, beam_seq, beam_sum, best_p, best_seq):
    """beam bookkeeping of position t in torch (caption_model.py beam_step + the finished-beam tracking), in place on the search's arrays:
    logp holds one row per live hypothesis -- ONE per sample at t = 0, where the hypothesis count grows from B to B * beam and the running
    sums are zero, `beam` per sample later -> (word_ix (B, beam), state_ix (B * beam,): the row each new hypothesis continues)."""
    B, beam, max_len = beam_seq.shape
    V1 = dec.vocab_size + 1
    nb = 1 if t == 0 else beam
    cand = logp.view(B, nb, -1)[:, :, :V1]
    if t > 0:
        cand = beam_sum.unsqueeze(-1) + cand
    ys, ix = _topk(cand.reshape(B, nb * V1).contiguous(), beam)
    beam_ix, word_ix = ix // V1, ix % V1
    if t > 0:
        beam_seq.copy_(beam_seq.gather(1, beam_ix.unsqueeze(-1).expand(-1, -1, max_len)))
    beam_seq[:, :, t] = word_ix
    beam_sum.copy_(ys)
    is_end = torch.ones_like(word_ix, dtype=torch.bool) if t == max_len - 1 else (word_ix == dec.eos_idx)
    # finished beams: keep, per sample, the best p seen so far (earlier / lower beam index wins ties)
    p_end = torch.where(is_end, beam_sum, torch.full_like(beam_sum, -float('inf')))
    pv, pi = p_end.max(dim=1)
    better = pv > best_p
    cand_seq = beam_seq.gather(1, pi.view(B, 1, 1).expand(-1, 1, max_len))[:, 0]
    best_seq.copy_(torch.where(better.unsqueeze(1), cand_seq, best_seq))
    best_p.copy_(torch.where(better, pv, best_p))
    beam_sum.sub_(1000.0 * is_end.to(F32))
    return word_ix, (beam_ix + base * nb).reshape(-1)


class _BeamSession(_Session):
    """The session of a beam search over B samples x `beam` hypotheses: the shared state plus the beam bookkeeping arrays."""

    def __init__(self, dec, B, beam, max_len, S, dev, slot=0, opts=None):
        super().__init__(dec, B, B * beam, max_len, S, dev, slot)
        self.beam = beam
        self.lists = _BeamLists(dec, B, beam, max_len, dev, opts, S) if opts is not None else None
        self.hist_attn = self.lists.hist_attn if self.lists is not None else None
        # position 0 runs for B rows (st0): its maps land here and go to slab 0 once per beam
        self.maps0 = torch.empty(1, B, self.hist_attn.shape[-1], dtype=F32, device=dev) if self.hist_attn is not None else None
        self.beam_seq = torch.zeros(B, beam, max_len, dtype=torch.long, device=dev)
        self.beam_sum = torch.zeros(B, beam, dtype=F32, device=dev)
        self.best_p = torch.empty(B, dtype=F32, device=dev)
        self.best_seq = torch.empty(B, max_len, dtype=torch.long, device=dev)
        self.base = torch.arange(B, device=dev).unsqueeze(1)

    def _book_kernel(self, last):
        """one launch (csrc/beam.hip): top-beam, sequence / cache-row-table / relational-memory reorder in place, finished-beam tracking,
        -1000 penalty, next input tokens -- and, between steps, the position counter's increment and the row table's next column"""
        st = self.st
        _beam_step(self.dec, self.logp_buf, self.beam, self.B, self.max_len, self.pos, last, self.beam_sum, self.beam_seq, self.best_p, self.best_seq,
                   self.words, st.mem32 if st.mem32 is not None else st.mem, st.mem[0].numel() * (2 if st.mem32 is not None else 1), st.anc,
                   None if last else self.pos, self.ticket, st.tmem if st.mem32 is None else None, self.lists)

    def _body(self):
        """positions 1 .. max_len-2: bookkeeping at position `pos` (which also advances it), then the decoder step that writes pos + 1"""
        self._book_kernel(False)
        self.st.step_static(self.words, self.pos, out=self.logp_buf, seed_rows=False)

    def _run_iter(self, enc, src_mask, return_scores=False, step_hook=None, burst=0):
        """run() as a generator that yields after every issued token step: a scheduler that drives several sessions (one per HIP stream)
        round-robin keeps all their launch queues fed (FineTune.generate_pipelined) -- issuing one session's ~3k launches in one go
        blocks the host at the GPU's pace, because a launch queue is finite.
        burst > 0 (and a replay plan, no step hook): yields -1 once everything in front of the token loop has been issued, then issues the
        loop `burst` steps per native call (evk_replay_run_n: no interpreter between the steps) -- the form a per-search host THREAD drives:
        ctypes drops the GIL for the call, so the thread may block on a full launch queue while the others keep issuing."""
        dec, B, beam, max_len, R = self.dec, self.B, self.beam, self.max_len, self.R
        dev, V1 = enc.device, dec.vocab_size + 1
        hook = step_hook if step_hook is not None else (lambda *a: None)
        model = dec.model
        src_mask = self._refill(enc, src_mask)
        st = self.st
        # ---- position 0: B rows, eagerly (modules/att_model.py:118-124: one decoder call with [BOS], then the features are tiled x beam)
        st0 = _DecoderState(dec, enc, src_mask, 1, cross_kv=(self.kc, self.vc))
        st.maps, st0.maps = self.hist_attn, self.maps0
        logp0 = st0.step(torch.full((B,), dec.bos_idx, dtype=torch.long, device=dev))            # (B, V+1)
        if self.hist_attn is not None:
            # every source row of position 0 is the study's one row, as _beam_first_position arranges the log-probability rows
            self.hist_attn[0].copy_(self.maps0[0].repeat_interleave(beam, 0))
        self.beam_seq.zero_()
        self.beam_sum.zero_()
        self.best_p.fill_(-float('inf'))
        self.best_seq.fill_(dec.pad_idx)
        if self.lists is not None:
            self.lists.reset()
            st.logit_scale = 1.0 / self.lists.opts['temperature']      # positions >= 1 only (att_model.py:119: position 0 is not scaled)
            self.beam_sum.fill_(-float('inf'))
            self.beam_sum[:, 0] = 0.0
            hook(0, logp0, self.beam_sum)
            _beam_first_position(dec, logp0, beam, B, max_len, self.beam_sum, self.beam_seq, self.best_p, self.best_seq, self.words, self.lists)
            word_ix = self.words.view(B, beam).clone()
            state_ix = self.base.expand(B, beam).reshape(-1)
        else:
            hook(0, logp0, self.beam_sum)
            word_ix, state_ix = _beam_book(dec, logp0, 0, self.base, self.beam_seq, self.beam_sum, self.best_p, self.best_seq)
        if max_len > 1:
            # the B -> B*beam expansion: every hypothesis inherits its sample's memory and position-0 keys / values
            ops.copy_kernel(st.mem, st0.mem.index_select(0, state_ix).contiguous())
            if st.mem32 is not None:
                ops.copy_kernel(st.mem32, st0.mem32.index_select(0, state_ix).contiguous())
            elif _RM_STEP[0]:
                if st.tmem is None:
                    st.tmem = torch.empty_like(st.mem)
                H.check(H.lib.evk_act_fwd(H.ptr(st.mem), H.ptr(st.tmem), st.mem.numel(), H.ACT_TANH, H.stream()), 'act_fwd')
            for i in range(len(st.ks)):
                st.ks[i][:, :1] = st0.ks[i][:, :1].index_select(0, state_ix)
                st.vs[i][:, :1] = st0.vs[i][:, :1].index_select(0, state_ix)
            self.pos.fill_(1)
            self.ticket.zero_()
            st.anc.copy_(st.rows.expand_as(st.anc))
            self.words.copy_(word_ix.reshape(-1))
            st.step_static(self.words, self.pos, out=self.logp_buf)             # writes position 1
            hook(1, self.logp_buf, self.beam_sum)
            # positions 1 .. max_len-2: body number i writes the log-probabilities of position i + 2
            yield from self._drive(max_len - 2, 2, step_hook, burst, (self.beam_sum,))
            self._book_kernel(True)                                      # t = max_len - 1: every live beam is closed
            _reap_plans()
        if self.lists is not None:
            return self.lists.result(return_scores)
        seq = self.best_seq.clone()
        if return_scores:
            return seq, self.best_p.clone()
        return seq


class _SampleSession(_Session):
    """The session of AttModel._sample over B samples x sample_n rows: the shared state with the identity row table (rows never trade
    places, so neither the caches nor the memory are permuted) plus the arrays of csrc/sample.hip.  The options are kernel arguments of the
    captured step, so they are part of the session's key (see sample())."""

    def __init__(self, dec, B, n, max_len, S, dev, opts, return_logprobs, slot=0, return_attention=False):
        super().__init__(dec, B, B * n, max_len, S, dev, slot)
        R, V1 = self.R, dec.vocab_size + 1
        self.nl = len(dec.model.decoder.layers)
        # the cross-attention maps of every step, slab t written by the step that computes position t (rows never trade places here)
        self.hist_attn = torch.zeros(max_len, R, self.nl * S, dtype=F32, device=dev) if return_attention else None
        self.opts = opts
        self.seq = torch.empty(R, max_len, dtype=torch.long, device=dev)
        self.unfinished = torch.empty(R, dtype=torch.uint8, device=dev)
        self.seq_logprobs = torch.empty(R, max_len, V1, dtype=F32, device=dev) if return_logprobs else None
        self.uniforms = torch.empty(R, max_len, dtype=F32, device=dev) if opts['method'] != 0 else None
        self.mem0 = None                  # the relational memory every row starts from

    def _book_kernel(self, last):
        """one launch (csrc/sample.hip): constraint, trigram penalty, stored row, choice, finished rows, next input tokens -- and, between
        steps, the position counter's increment"""
        _sample_step(self.dec, self.logp_buf, self.pos, self.seq, self.unfinished, self.words, self.seq_logprobs, self.uniforms, self.opts,
                     self.B, None if last else self.pos, self.ticket)

    def _body(self):
        """the choice at position `pos` (which also advances it), then the decoder step that reads the chosen words at pos + 1"""
        self._book_kernel(False)
        self.st.step_static(self.words, self.pos, out=self.logp_buf, seed_rows=False)

    def _run_iter(self, enc, src_mask, uniforms=None, step_hook=None, burst=0):
        """as _BeamSession._run_iter (same yields, same burst protocol) -> (seq, seq_logprobs or None [, attention])"""
        dec, max_len = self.dec, self.max_len
        hook = step_hook if step_hook is not None else (lambda *a: None)
        self._refill(enc, src_mask)
        st = self.st
        st.maps = self.hist_attn
        # ---- every row starts from the initial memory and [BOS] at position 0 (att_model.py:157-173)
        if self.mem0 is None or self.mem0.shape != st.mem.shape:
            self.mem0 = dec.model.rm.init_memory(self.R, enc.device).to(st.mem.dtype).contiguous()
            self.mem0_32 = self.mem0.float().contiguous()
        st.mem.copy_(self.mem0)
        if st.mem32 is not None:
            st.mem32.copy_(self.mem0_32)
        elif _RM_STEP[0]:
            if st.tmem is None:
                st.tmem = torch.empty_like(st.mem)
            H.check(H.lib.evk_act_fwd(H.ptr(st.mem), H.ptr(st.tmem), st.mem.numel(), H.ACT_TANH, H.stream()), 'act_fwd')
        self.seq.fill_(dec.pad_idx)
        self.unfinished.fill_(1)
        if self.seq_logprobs is not None:
            self.seq_logprobs.zero_()
        if self.uniforms is not None:
            self.uniforms.copy_(uniforms)
        self.pos.zero_()
        self.ticket.zero_()
        self.words.fill_(dec.bos_idx)
        st.step_static(self.words, self.pos, out=self.logp_buf)              # position 0 (the row table stays the identity it was built as)
        hook(0, self.logp_buf)
        # positions 0 .. max_len-2: body number i chooses the word of position i and writes the log-probabilities of position i + 1
        yield from self._drive(max_len - 1, 1, step_hook, burst)
        self._book_kernel(True)                                               # the last position: nothing follows it
        _reap_plans()
        out = (self.seq.clone(), (self.seq_logprobs.clone() if self.seq_logprobs is not None else None))
        if self.hist_attn is not None:
            # the history transposed to rows first; a row that has emitted [EOS] (or [PAD]) keeps stepping: its later maps are zeroed
            ended = (self.seq == dec.eos_idx) | (self.seq == dec.pad_idx)
            live = (ended.cumsum(1) - ended.long()) == 0                       # no end mark in front of position t
            att = self.hist_attn.permute(1, 0, 2).reshape(self.R, max_len, self.nl, -1)
            out = out + (att * live.view(self.R, max_len, 1, 1).to(F32),)
        return out


def _sample_step(dec, logp, pos, seq, unfinished, words, seq_logprobs, uniforms, opts, block_rows, pos_advance, ticket):
    H.check(H.lib.evk_sample_step(H.ptr(logp), logp.stride(0), dec.vocab_size + 1, seq.shape[0], seq.shape[1], H.ptr(pos), dec.eos_idx, dec.pad_idx,
                                  block_rows if opts['block_trigrams'] else 0, int(opts['decoding_constraint']), C.c_float(opts['temperature']),
                                  opts['method'], C.c_float(opts['param']), H.ptr(seq), H.ptr(unfinished), H.ptr(words),
                                  H.ptr(seq_logprobs) if seq_logprobs is not None else None, H.ptr(uniforms) if uniforms is not None else None,
                                  H.ptr(pos_advance), H.ptr(ticket), H.stream()), 'sample_step')


_SESSIONS = weakref.WeakKeyDictionary()          # decoder module -> {key: session}, the most recently used last


def _session_ok(dec, args):
    """the session serves this geometry (its kernels read the self-attention caches through the row table: head dim 64, <= 256 positions)"""
    model = dec.model
    h = model.decoder.layers[0].self_attn.h
    return _SESSION[0] and model.d_model // h == 64 and int(args['max_seq_len']) <= 256


def _attention_ok(dec, args, S):
    """attention maps come out of the session's cross-attention kernel (evk_decode_attention_maps): refuse, with the reason, what it does not
    serve"""
    model = dec.model
    h = model.decoder.layers[0].self_attn.h
    why = None
    if not _SESSION[0]:
        why = 'the decode session is switched off (EVK_DECODE_SESSION=0)'
    elif model.d_model // h != 64:
        why = 'the head size is %d, the kernel serves 64' % (model.d_model // h)
    elif int(args['max_seq_len']) > 256:
        why = 'max_seq_len %d exceeds the 256 positions of the session' % int(args['max_seq_len'])
    elif S > 256:
        why = '%d encoder tokens exceed the 256 keys of the kernel' % S
    if why is not None:
        raise NotImplementedError('return_attention needs the decode session and its cross-attention kernel: ' + why)


def _session_for(dec, key, make):
    """the decoder's session under `key`, built by make() on first use.  A few batch geometries / slots at most (each holds its caches:
    6 x R x max_len x 512 x 2 B), the least recently used evicted first.  A generator still in flight keeps its evicted session alive, whose
    plan is then destroyed behind a device synchronisation: keep EVK_DECODE_DEPTH times the batch geometries in use at 6 or below."""
    sessions = _SESSIONS.setdefault(dec, {})
    ses = sessions.pop(key, None)
    if ses is None:
        ses = make()
        while len(sessions) >= 6:
            sessions.pop(next(iter(sessions)))
    sessions[key] = ses
    return ses


@torch.no_grad()
def beam_search(dec, enc_states, enc_mask, args, return_scores=False, step_hook=None, slot=0, as_iterator=False, burst=0, return_logprobs=False,
                return_attention=False):
    """AttModel._sample_beam (modules/att_model.py:98-137) -> seq (rows, max_seq_len) int64 token ids padded with [PAD]; with return_logprobs
    (seq, seq_logprobs (rows, max_seq_len, V+1) f32: the log-probability row every word was selected from, after temperature and constraint,
    zero beyond the hypothesis's length); with return_scores the list scores (rows,) come last (f32 running sums on the plain route, f64
    after the length penalty once an option is set).  rows = B * sample_n.  Options read from `args` (beam_options): temperature (positions
    >= 1), decoding_constraint, length_penalty ('' | 'avg_<x>' | 'wu_<alpha>'), sample_n (1: the best finished hypothesis of each study;
    beam_size: all `beam_size` entries of its finished list, next to each other in list order).  With every option at its default and no
    log-probabilities the search issues exactly the launches it issued before the options existed.
    return_attention: the result gains `attention` f32 (rows, max_seq_len, n_layers, S) after seq (and seq_logprobs), before the scores: for
    every word the head-mean cross-attention weights over the S encoder tokens, one map per decoder layer (the reference's
    decoder.layers[i].src_attn.attn, encoder_decoder.py:189,200, averaged over the heads), rows in the order of seq, zeros beyond a
    hypothesis's length.  The maps come out of the cross-attention launch of the token step (evk_decode_attention_maps): the step keeps its
    launch count.  Needs the session (head size 64, S <= 256, max_seq_len <= 256, EVK_DECODE_SESSION on): NotImplementedError otherwise.
    step_hook(t, logp, beam_sum): test instrument, called on the launching stream right before the bookkeeping of position t consumes
    `logp` (f32, one row of >= V+1 log-probabilities per live hypothesis; may be edited in place) with the running sums (B, beam).
    slot: which of the decoder's persistent sessions to use (searches that are in flight at the same time need different slots);
    as_iterator: return a generator that yields after every issued token step and returns the result (see _BeamSession.run_iter);
    burst: with as_iterator, token steps per native call (see _BeamSession._run_iter)."""
    beam, max_len = int(args.get('beam_size', 3)), int(args['max_seq_len'])
    opts = beam_options(args, beam, return_logprobs, return_attention)
    if beam < 1 or beam > 8 or beam > dec.vocab_size + 1:
        raise ValueError('beam_size must be in [1, 8]')
    session = _session_ok(dec, args)
    if as_iterator and not session:
        raise NotImplementedError('stepwise beam search needs the session path')
    was_training = dec.training
    dec.eval()
    try:
        enc, src_mask = dec.encode(enc_states, enc_mask)
        if return_attention:
            _attention_ok(dec, args, enc.shape[1])
        if not session:
            return _beam_eager(dec, enc, src_mask, beam, max_len, opts, return_scores, step_hook)
        B, S, dev = enc.shape[0], enc.shape[1], enc.device
        key = (B, beam, max_len, S, dev.index, src_mask is None, slot)
        if opts is not None:
            key = key + (tuple(sorted(opts.items())),)
        ses = _session_for(dec, key, lambda: _BeamSession(dec, B, beam, max_len, S, dev, slot, opts))
        if as_iterator:
            return ses.run_iter(enc, src_mask, return_scores, step_hook, burst)
        return ses.run(enc, src_mask, return_scores, step_hook)
    finally:
        dec.train(was_training)


SAMPLE_GREEDY, SAMPLE_ALL, SAMPLE_TOPK, SAMPLE_TOPP = 0, 1, 2, 3           # the method codes of evk_sample_step


def parse_sample_method(sample_method):
    """CaptionModel.sample_next_word's reading of `sample_method` (caption_model.py:363-398) -> (method code of evk_sample_step, parameter):
    'greedy'; 'top<k>' with k >= 1; 'top<p>' with 0 < p < 1; every other name ('sample', and 'beam_search' once beam_size is 1) draws from
    the unfiltered distribution, as the reference's final `else` does.  'gumbel' is not on the path."""
    if sample_method == 'greedy':
        return SAMPLE_GREEDY, 0.0
    if sample_method == 'gumbel':
        raise NotImplementedError("sample_method 'gumbel' (gumbel-softmax sampling) is not on the path")
    if sample_method.startswith('top'):
        top_num = float(sample_method[3:])
        if 0 < top_num < 1:
            return SAMPLE_TOPP, top_num
        if int(top_num) < 1:
            raise ValueError('sample_method %r: k must be at least 1' % sample_method)
        return SAMPLE_TOPK, float(int(top_num))
    return SAMPLE_ALL, 0.0


@torch.no_grad()
def sample(dec, enc_states, enc_mask, args, return_logprobs=False, step_hook=None, uniforms=None, slot=0, as_iterator=False, burst=0,
           return_attention=False):
    """AttModel._sample (modules/att_model.py:139-224) -> (seq (R, max_seq_len) int64 padded with [PAD], seq_logprobs (R, max_seq_len, V+1)
    f32 or None), R = B * sample_n rows with the sample_n copies of a study next to each other.  Options read from `args`: sample_method
    (parse_sample_method), temperature, sample_n, decoding_constraint, block_trigrams -- the reference blocks only the first B of the R rows
    (its loop runs over batch_size), and so does this.  Always max_seq_len steps without a host synchronisation: rows that have emitted [EOS]
    continue as [PAD] with zero log-probability rows, which is what the reference's early exit returns.
    uniforms: (R, max_seq_len) f32 in [0, 1), one per row and position, for the stochastic methods (default: torch.rand on the device, from
    args['generator'] if given); step_hook(t, logp): test instrument, called on the launching stream right before the choice at position t
    consumes `logp` (f32 (R, >= V+1), may be edited in place); slot / as_iterator / burst: as beam_search.
    return_attention: the result is (seq, seq_logprobs, attention), attention f32 (R, max_seq_len, n_layers, S) as beam_search returns it
    (rows never trade places on this route: the step history transposed), zeros at the positions after a row's [EOS]; same conditions,
    same NotImplementedError."""
    was_training = dec.training
    dec.eval()
    try:
        max_len, n = int(args['max_seq_len']), int(args.get('sample_n', 1))
        if args.get('group_size', 1) != 1:
            raise NotImplementedError("diverse sampling / diverse beam search (group_size > 1, AttModel._diverse_sample) is not on the path: the "
                                      "reference's own grouped search fails (CaptionModel.beam_search calls self.repeat_tensor, which no class defines)")
        if n < 1:
            raise ValueError('sample_n must be at least 1')
        method, param = parse_sample_method(args.get('sample_method', 'greedy'))
        temperature = float(args.get('temperature', 1.0))
        if method != SAMPLE_GREEDY and not temperature > 0:
            raise ValueError('temperature must be positive')
        if method == SAMPLE_TOPK and param > dec.vocab_size + 1:
            raise ValueError('top-k: k exceeds the vocabulary')
        opts = dict(method=method, param=param, temperature=temperature, decoding_constraint=int(bool(args.get('decoding_constraint', 0))),
                    block_trigrams=int(bool(args.get('block_trigrams', 0))))
        enc, src_mask = dec.encode(enc_states, enc_mask)
        B, S, dev = enc.shape[0], enc.shape[1], enc.device
        R = B * n
        if method != SAMPLE_GREEDY:
            if uniforms is None:
                uniforms = torch.rand(R, max_len, dtype=F32, device=dev, generator=args.get('generator'))
            if tuple(uniforms.shape) != (R, max_len):
                raise ValueError('uniforms must be (%d, %d)' % (R, max_len))
            uniforms = uniforms.to(device=dev, dtype=F32)
        if return_attention:
            _attention_ok(dec, args, S)
        if not _session_ok(dec, args):
            if as_iterator:
                raise NotImplementedError('stepwise sampling needs the session path')
            return _sample_eager(dec, enc, src_mask, max_len, n, opts, return_logprobs, step_hook, uniforms)
        # ('sample' in front: a beam session's key starts with an integer)
        key = ('sample', B, n, max_len, S, dev.index, src_mask is None, slot, bool(return_logprobs), tuple(sorted(opts.items())))
        if return_attention:
            key = key + ('attention',)
        ses = _session_for(dec, key, lambda: _SampleSession(dec, B, n, max_len, S, dev, opts, return_logprobs, slot, bool(return_attention)))
        if as_iterator:
            return ses.run_iter(enc, src_mask, uniforms, step_hook, burst)
        return ses.run(enc, src_mask, uniforms, step_hook)
    finally:
        dec.train(was_training)


def _sample_eager(dec, enc, src_mask, max_len, n, opts, return_logprobs, step_hook, uniforms):
    """sample() without the persistent session (head dims other than 64, max_seq_len > 256, or EVK_DECODE_SESSION=0): the decoder steps
    run eagerly with the position on the host; the choice is the same kernel."""
    B, dev, V1 = enc.shape[0], enc.device, dec.vocab_size + 1
    R = B * n
    cross = ([l.src_attn.linears[1](enc) for l in dec.model.decoder.layers], [l.src_attn.linears[2](enc) for l in dec.model.decoder.layers])
    st = _DecoderState(dec, enc, src_mask, max_len, cross_kv=cross, rows=R)
    if n > 1:
        st.expand_cross(n)
    seq = torch.full((R, max_len), dec.pad_idx, dtype=torch.long, device=dev)
    unfinished = torch.ones(R, dtype=torch.uint8, device=dev)
    words = torch.full((R,), dec.bos_idx, dtype=torch.long, device=dev)
    seq_logprobs = torch.zeros(R, max_len, V1, dtype=F32, device=dev) if return_logprobs else None
    pos = torch.zeros(1, dtype=torch.long, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    for t in range(max_len):
        logp = st.step(words)
        if step_hook is not None:
            step_hook(t, logp)
        _sample_step(dec, logp, pos, seq, unfinished, words, seq_logprobs, uniforms, opts, B, pos, ticket)
    return seq, seq_logprobs


def _beam_eager(dec, enc, src_mask, beam, max_len, opts, return_scores, step_hook):
    """beam_search() without the persistent session (head dims other than 64, max_seq_len > 256, or EVK_DECODE_SESSION=0): the decoder
    steps run eagerly with the position on the host, the bookkeeping in torch, and the self-attention caches themselves are re-ordered.
    The options (beam_options) are arguments of the session's bookkeeping kernel and are refused here."""
    if opts is not None:
        raise NotImplementedError('beam search options (temperature, decoding_constraint, length_penalty, sample_n, log-probabilities) '
                                  'need the fused bookkeeping kernel and the cache row table (head dim 64, max_seq_len <= 256)')
    B, dev = enc.shape[0], enc.device
    st = _DecoderState(dec, enc, src_mask, max_len)
    base = torch.arange(B, device=dev).unsqueeze(1)
    beam_seq = torch.zeros(B, beam, max_len, dtype=torch.long, device=dev)
    beam_sum = torch.zeros(B, beam, dtype=F32, device=dev)
    best_p = torch.full((B,), -float('inf'), dtype=F32, device=dev)
    best_seq = torch.full((B, max_len), dec.pad_idx, dtype=torch.long, device=dev)
    words = torch.full((B,), dec.bos_idx, dtype=torch.long, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for t in range(max_len):
        logp = st.step(words)
        if step_hook is not None:
            step_hook(t, logp, beam_sum)
        word_ix, state_ix = _beam_book(dec, logp, t, base, beam_seq, beam_sum, best_p, best_seq)
        words = word_ix.reshape(-1)
        if t + 1 < max_len:
            st.reorder(state_ix)
        if t == 0:
            st.expand_cross(beam)
            ev0.record()
    ev1.record()
    stats.update(step_events=(ev0, ev1, max_len - 1), step_launches=None, graph=False, replayer=False, fused_bookkeeping=False)
    if return_scores:
        return best_seq, best_p
    return best_seq


def attention_grid(attention, grid_hw):
    """Split attention maps over the image tokens (..., S) into (global, patches): `global` (...,) is the weight of token 0, `patches`
    (..., gh, gw) the remaining S - 1 weights on the trunk's feature map.  The token layout is the anchor view's, as _image_tokens produces
    it: the global (patch-mean) token first, then the patches in row-major order -- the layout FineTune.generate_with_attention returns.  (The
    maps of beam_search / sample themselves cover what the decoder attends to: it drops the global token, so they hold the gh * gw patch
    columns only; generate_with_attention puts an exact zero in front.)  ValueError if gh * gw != S - 1."""
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    S = attention.shape[-1]
    if gh < 1 or gw < 1 or gh * gw != S - 1:
        raise ValueError('attention_grid: a %d x %d grid does not hold the %d patch tokens of maps over %d tokens' % (gh, gw, S - 1, S))
    return attention[..., 0], attention[..., 1:].reshape(*attention.shape[:-1], gh, gw)
