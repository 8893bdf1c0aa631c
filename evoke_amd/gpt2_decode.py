"""Device-resident beam search of the distilgpt2 decoder backend (evoke_amd/gpt2.py): what decode._BeamSession is for the R2Gen decoder.

The whole Hugging Face beam search (classic BeamSearchScorer, length_penalty 1, early_stopping False: language_model.py:271-280 through
`generate`, restated in oracle/gpt2.py:120-186) runs as a captured per-token step with no host synchronisation inside the token loop:
  * evk_hf_beam_step (csrc/hf_beam.hip): candidates, rank walk, hypothesis lists, done flags, sequence / cache-row-table permutation,
    next tokens, position counter -- one launch;
  * a static GPT-2 step: embedding at the device-held position, per block ln_1 -> fused c_attn -> single-query self-attention with fused
    K / V append over the row table (evk_decode_attention_qkv at head size 64, evk_decode_attention_wide at 128 / 256) -> c_proj +
    residual -> ln_cross_attn -> q_attn -> cross-attention (one K / V row per study, kv_div = beam) -> c_proj + residual -> ln_2 -> MLP
    (gelu_new); ln_f, the tied head into a persistent f32 buffer, log_softmax.
The session (caches, row table, cross K / V, hypothesis arrays, captured step, replay plan) lives on the decoder and is reused by every
batch of its geometry; decode._Session._drive supplies warm-up, capture, replay and burst yields.

_GPT2SampleSession is the same for Hugging Face's sampling / greedy decoding with logits processors (num_beams 1): the same GPT-2 step
without the log_softmax, and evk_hf_sample_step (csrc/hf_sample.hip) on the raw logits in place of evk_hf_beam_step.

_GPT2BeamOptionsSession is the beam session with Hugging Face's repetition_penalty / no_repeat_ngram_size / min_length processors on the
log-probability rows and the scorer's length_penalty / early_stopping: the same captured step with evk_hf_beam_step_opts as its bookkeeping
launch -- one launch still, so a step keeps the plain beam step's launch count."""
import ctypes as C
import math
from collections import deque

import torch

from . import decode
from . import hip as H
from . import ops
from .config import tunable
from .ops import BF16, F32

_POLL = [True]           # stop issuing steps once a completed copy of the done counter says every study is done (False: always max_seq_len steps)
POLL_EVERY = 8           # issued steps between two non-blocking copies of the done counter


def session_usable(dec, S=None, need_graph=True):
    """the device route serves this decoder (and an encoder output of S positions); need_graph: only while graph capture is enabled (the
    beam search then has its host-driven route; the sampling route has none and issues its steps eagerly instead)"""
    d = dec.gpt2.transformer.wte.weight.shape[1]
    return (d % dec.heads == 0 and d // dec.heads in (64, 128, 256) and 5 <= int(dec.max_seq_len) <= 256 and
            (decode._GRAPH_ENABLED[0] or not need_graph) and (S is None or S <= 256) and tunable('EVK_GPT2_SESSION', '1') != '0')


def _attend(q, ldq, k, v, knew, vnew, rowmap, last_pos, R, S, heads, dh, kv_div):
    """single-query attention -> (R, 1, heads * dh); q: tensor or raw pointer of rows with leading dimension ldq"""
    out = torch.empty(R, 1, heads * dh, dtype=BF16, device=k.device)
    scale = C.c_float(1.0 / math.sqrt(dh))
    if dh != 64:
        H.check(H.lib.evk_decode_attention_wide(q, ldq, H.ptr(k), H.ptr(v), knew, vnew, None, H.ptr(rowmap), H.ptr(last_pos), H.ptr(out), R, S, heads,
                                                dh, kv_div, scale, H.stream()), 'decode_attention_wide')
    elif knew is not None:
        H.check(H.lib.evk_decode_attention_qkv(q, ldq, H.ptr(k), H.ptr(v), H.ptr(rowmap), H.ptr(last_pos), H.ptr(out), R, S, heads, dh, scale,
                                               H.stream()), 'decode_attention_qkv')
    else:
        H.check(H.lib.evk_decode_attention(q, H.ptr(k), H.ptr(v), None, H.ptr(out), R, S, heads, dh, kv_div, scale, H.stream()), 'decode_attention')
    return out


class _GPT2Session(decode._Session):
    """The session of a distilgpt2 beam search over B studies x nb beams: self-attention caches and their row table, cross-attention K / V,
    the log-probability buffer, position counter and ticket, the running beams and the hypothesis lists of evk_hf_beam_step."""
    route = 'beam'                       # what decode.stats['gpt2_route'] reports

    def __init__(self, dec, B, nb, max_len, S, dev, slot=0, n_return=1):
        # (decode._Session.__init__ sizes its buffers from the R2Gen model: this backend allocates its own and shares the driving code)
        self._init_driving(dec, slot)
        t = dec.gpt2.transformer
        d, nl, V = t.wte.weight.shape[1], len(t.h), dec.vocab
        R = B * nb
        self.B, self.nb, self.R, self.max_len, self.S, self.n_return = B, nb, R, max_len, S, n_return
        self.d, self.heads, self.dh, self.V = d, dec.heads, d // dec.heads, V
        self.kc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.vc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.ks = [torch.zeros(R, max_len, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.vs = [torch.zeros(R, max_len, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.anc0 = torch.arange(R, dtype=torch.int32, device=dev).view(R, 1).expand(R, max_len).contiguous()
        self.anc = self.anc0.clone()
        self.words = torch.empty(R, dtype=torch.long, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.logits_buf = torch.zeros(R, (V + 7) // 8 * 8, dtype=F32, device=dev)      # (pad columns zeroed once)
        self.logp_buf = torch.empty(R, V, dtype=F32, device=dev)
        self.scores0 = torch.zeros(B, nb, dtype=F32, device=dev)
        self.scores0[:, 1:] = -1e9                                                     # all rows start from [BOS]: only the first may win
        self.scores = self.scores0.clone()
        self.seqs = torch.empty(R, max_len, dtype=torch.long, device=dev)
        self.hyp_score = torch.empty(B, nb, dtype=torch.float64, device=dev)
        self.hyp_len = torch.empty(B, nb, dtype=torch.int32, device=dev)
        self.hyp_seq = torch.empty(B, nb, max_len, dtype=torch.long, device=dev)
        self.done = torch.empty(B, dtype=torch.uint8, device=dev)
        self.n_done = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pin = torch.empty(max_len // POLL_EVERY + 4, dtype=torch.int32).pin_memory()
        self.weights_key = None

    def _book(self, last):
        """one launch (csrc/hf_beam.hip): everything between two decoder steps, and -- between steps -- the position counter's increment"""
        dec = self.dec
        H.check(H.lib.evk_hf_beam_step(H.ptr(self.logp_buf), self.logp_buf.stride(0), self.V, self.nb, self.B, self.max_len, H.ptr(self.pos),
                                       dec.eos_token_id, dec.pad_token_id, int(last), H.ptr(self.scores), H.ptr(self.seqs), H.ptr(self.words),
                                       H.ptr(self.anc), self.anc.shape[1], H.ptr(self.hyp_score), H.ptr(self.hyp_len), H.ptr(self.hyp_seq),
                                       H.ptr(self.done), H.ptr(self.n_done), None if last else H.ptr(self.pos), H.ptr(self.ticket), H.stream()),
                'hf_beam_step')

    def _trunk(self):
        """the GPT-2 block stack and the tied head for the tokens in `words` at position *pos -> logits_buf (f32); no host-side shape depends
        on the step index.  Shared with _GPT2SampleSession, whose bookkeeping reads the raw logits"""
        t = self.dec.gpt2.transformer
        R, d, heads, dh, nb = self.R, self.d, self.heads, self.dh, self.nb
        x = ops.embedding(self.words.view(R, 1), t.wte.weight, pos=t.wpe.weight, pos0=self.pos)
        for i, blk in enumerate(t.h):
            qkv = blk.attn.c_attn(blk.ln_1(x))                           # (R, 1, 3 d): q | k | v
            base = qkv.data_ptr()
            a = _attend(base, 3 * d, self.ks[i], self.vs[i], base + 2 * d, base + 4 * d, self.anc, self.pos, R, self.max_len, heads, dh, 1)
            x = blk.attn.c_proj(a, resid=x)
            q = blk.crossattention.q_attn(blk.ln_cross_attn(x))
            a = _attend(q.data_ptr(), 0, self.kc[i], self.vc[i], None, None, None, None, R, self.S, heads, dh, nb)
            x = blk.crossattention.c_proj(a, resid=x)
            f = ops.activation(blk.mlp.c_fc(blk.ln_2(x)), H.ACT_GELU_NEW)
            x = blk.mlp.c_proj(f, resid=x)
        h = t.ln_f(x)
        W, V, Np = self.dec.gpt2.lm_head.weight, self.V, self.logits_buf.shape[1]
        ops.gemm(h, ops.shadow(W, pad_rows=(V != Np)), self.logits_buf, R, V, d, lda=d, ldb=d, ldc=Np)

    def _step(self):
        """_trunk, then the log-probabilities the beam bookkeeping reads -> logp_buf"""
        self._trunk()
        ops.log_softmax(self.logits_buf, self.V, out=self.logp_buf)

    def _body(self):
        """bookkeeping of position `pos` (which also advances it), then the decoder step that writes the log-probabilities of pos + 1"""
        self._book(False)
        self._step()

    def _refill_cross(self, enc):
        """cross-attention K / V of this batch into the session's buffers; a captured step whose weights have changed since is retired"""
        dec, d = self.dec, self.d
        for i, blk in enumerate(dec.gpt2.transformer.h):
            ck, cv = blk.crossattention.c_attn(enc).split(d, dim=2)
            ops.copy_kernel(self.kc[i], ck.contiguous())
            ops.copy_kernel(self.vc[i], cv.contiguous())
        ps = list(dec.parameters())
        key = (ops.WEIGHT_EPOCH[0], tuple(p._version for p in ps), ps[0].data_ptr())
        if key != self.weights_key:
            self._retire_plan()
            self.weights_key = key

    def _refill(self, enc):
        """_refill_cross, and the search state back to [BOS]"""
        dec = self.dec
        self._refill_cross(enc)
        self.seqs.fill_(dec.pad_token_id)
        self.seqs[:, 0] = dec.bos_token_id
        self.words.fill_(dec.bos_token_id)
        self.scores.copy_(self.scores0)
        self.anc.copy_(self.anc0)
        self.pos.zero_()
        self.ticket.zero_()
        self.hyp_score.fill_(-float('inf'))
        self.hyp_len.zero_()
        self.hyp_seq.fill_(dec.pad_token_id)
        self.done.zero_()
        self.n_done.zero_()

    def _n_units(self):
        """what the done counter counts up to: studies"""
        return self.B

    def _stopper(self):
        """-> stop(i) for _drive: every POLL_EVERY issued steps the done counter is copied to pinned memory without blocking and an event
        recorded; the newest copy whose event has completed decides.  Done studies are frozen (csrc/hf_beam.hip), so steps issued after
        the last study became done cannot change the result."""
        polls, state, B = deque(), dict(last=0, slot=0), self._n_units()

        def stop(i):
            if not _POLL[0]:
                return False
            seen = None
            while polls and polls[0][1].query():
                seen = polls.popleft()[0]
            if seen is not None and int(self.pin[seen]) == B:
                return True
            if i - state['last'] >= POLL_EVERY and state['slot'] < self.pin.numel():
                j = state['slot']
                self.pin[j:j + 1].copy_(self.n_done, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                polls.append((j, ev))
                state['last'], state['slot'] = i, j + 1
            return False
        return stop

    def _run_iter(self, enc, return_scores=False, step_hook=None, burst=0):
        """-> packed (B * n, max_len + 1) int64: the first n list entries of every study next to each other, padded with [PAD], the last
        column their length in columns (unpack() trims) [, scores (B * n,) f64].  Yields as decode._BeamSession._run_iter does."""
        B, nb, n, max_len = self.B, self.nb, self.n_return, self.max_len
        hook = step_hook if step_hook is not None else (lambda *a: None)
        self._refill(enc)
        self._step()                                                     # position 0: every row reads [BOS]
        hook(0, self.logp_buf, self.scores)
        # body number i consumes the log-probabilities of position i and writes those of position i + 1
        yield from self._drive(max_len - 2, 1, step_hook, burst, (self.scores,), stop=self._stopper())
        self._book(True)                                                 # the last position: every study that is not done closes its beams
        decode._reap_plans()
        decode.stats['gpt2_steps_issued'] = self.issued + 1
        decode.stats['gpt2_route'] = self.route
        packed = torch.cat([self.hyp_seq[:, :n].reshape(B * n, max_len), self.hyp_len[:, :n].reshape(B * n, 1).long()], dim=1)
        if return_scores:
            return packed, self.hyp_score[:, :n].reshape(-1).clone()
        return packed


BEAM_NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, length_penalty=1.0, early_stopping=False)


def length_divisors(length_penalty, max_len):
    """D[c] = c ** length_penalty for c = 0 .. max_len as Python floats (what HF's scorer divides a sum by at cur_len = c; D[0] is never
    read): computed here and handed to the kernel as f64, so that a score is the quotient a host restatement computes"""
    lp = float(length_penalty)
    return [(float(c) ** lp) if c or lp >= 0 else float('inf') for c in range(max_len + 1)]


class _GPT2BeamOptionsSession(_GPT2Session):
    """_GPT2Session whose bookkeeping launch is evk_hf_beam_step_opts: the three logits processors on the running beams' rows (in place
    in logp_buf, which log_softmax rewrites every step) and the scorer's length_penalty / early_stopping.  The options are kernel arguments
    of the captured step, so they are part of the session's key (see search()).  Everything else is the beam session's."""
    route = 'beam-options'

    def __init__(self, dec, B, nb, max_len, S, dev, opts, slot=0, n_return=1):
        super().__init__(dec, B, nb, max_len, S, dev, slot, n_return)
        self.opts = dict(opts)
        lp = float(self.opts['length_penalty'])
        self.len_div = None if lp == 1.0 else torch.tensor(length_divisors(lp, max_len), dtype=torch.float64, device=dev)

    def _book(self, last):
        dec, o = self.dec, self.opts
        H.check(H.lib.evk_hf_beam_step_opts(H.ptr(self.logp_buf), self.logp_buf.stride(0), self.V, self.nb, self.B, self.max_len, H.ptr(self.pos),
                                            dec.eos_token_id, dec.pad_token_id, int(last), H.ptr(self.scores), H.ptr(self.seqs),
                                            H.ptr(self.words), H.ptr(self.anc), self.anc.shape[1], H.ptr(self.hyp_score), H.ptr(self.hyp_len),
                                            H.ptr(self.hyp_seq), H.ptr(self.done), H.ptr(self.n_done), None if last else H.ptr(self.pos),
                                            H.ptr(self.ticket), C.c_float(o['repetition_penalty']), int(o['no_repeat_ngram_size']),
                                            int(o['min_length']), H.ptr(self.len_div) if self.len_div is not None else None,
                                            int(bool(o['early_stopping'])), H.stream()), 'hf_beam_step_opts')


class _GPT2SampleSession(_GPT2Session):
    """The session of Hugging Face's sampling / greedy decoding with logits processors over B studies x n rows: the GPT-2 step of the beam
    session (the n copies of a study next to each other share the study's cross-attention K / V, kv_div = n; rows never trade places, so the
    cache row table stays the identity) plus the arrays of evk_hf_sample_step (csrc/hf_sample.hip), which reads the raw logits: no
    log_softmax launch.  The options are kernel arguments of the captured step, so they are part of the session's key (see sample())."""

    def __init__(self, dec, B, n, max_len, S, dev, opts, with_logp=False, slot=0, keep_rows=False):
        self._init_driving(dec, slot)
        t = dec.gpt2.transformer
        d, nl, V = t.wte.weight.shape[1], len(t.h), dec.vocab
        R = B * n
        self.B, self.nb, self.R, self.max_len, self.S, self.n_return = B, n, R, max_len, S, n          # (nb: rows per study, read by _trunk)
        self.d, self.heads, self.dh, self.V = d, dec.heads, d // dec.heads, V
        self.opts = dict(opts)
        self.kc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.vc = [torch.empty(B, S, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.ks = [torch.zeros(R, max_len, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.vs = [torch.zeros(R, max_len, d, dtype=BF16, device=dev) for _ in range(nl)]
        self.anc = torch.arange(R, dtype=torch.int32, device=dev).view(R, 1).expand(R, max_len).contiguous()
        self.words = torch.empty(R, dtype=torch.long, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)
        self.logits_buf = torch.zeros(R, (V + 7) // 8 * 8, dtype=F32, device=dev)      # (pad columns zeroed once, never read by the bookkeeping)
        self.logp_buf = self.logits_buf[:, :V]                                         # what _drive hands to a step hook: the raw logits
        self.seqs = torch.empty(R, max_len, dtype=torch.long, device=dev)
        self.unfinished = torch.empty(R, dtype=torch.uint8, device=dev)
        self.n_done = torch.zeros(1, dtype=torch.int32, device=dev)
        self.uniforms = torch.empty(R, max_len, dtype=F32, device=dev) if opts['do_sample'] else None
        self.tok_logp = torch.empty(R, max_len, dtype=F32, device=dev) if with_logp else None
        self.rows_out = torch.empty(max_len, R, V, dtype=F32, device=dev) if keep_rows else None
        self.pin = torch.empty(max_len // POLL_EVERY + 4, dtype=torch.int32).pin_memory()
        self.weights_key = None

    def _n_units(self):
        """the done counter counts rows"""
        return self.R

    def _book(self, last):
        """one launch (csrc/hf_sample.hip): processors, choice, finished rows, next tokens, and -- between steps -- the position counter's
        increment"""
        dec, o = self.dec, self.opts
        H.check(H.lib.evk_hf_sample_step(H.ptr(self.logits_buf), self.logits_buf.stride(0), self.V, self.R, self.max_len, H.ptr(self.pos),
                                         dec.eos_token_id, dec.pad_token_id, int(bool(o['do_sample'])), C.c_float(o['repetition_penalty']),
                                         int(o['no_repeat_ngram_size']), int(o['min_length']), C.c_float(o['temperature']), int(o['top_k']),
                                         C.c_float(o['top_p']), H.ptr(self.seqs), H.ptr(self.unfinished), H.ptr(self.words), H.ptr(self.n_done),
                                         H.ptr(self.tok_logp) if self.tok_logp is not None else None,
                                         H.ptr(self.rows_out) if self.rows_out is not None else None,
                                         H.ptr(self.uniforms) if self.uniforms is not None else None,
                                         None if last else H.ptr(self.pos), H.ptr(self.ticket), H.stream()), 'hf_sample_step')

    def _body(self):
        """the choice of column pos + 1 (which also advances pos), then the decoder step that writes the logits of the column after it"""
        self._book(False)
        self._trunk()

    def _refill(self, enc, uniforms=None, generator=None):
        """_refill_cross, every row back to [BOS], fresh uniform numbers (the captured step reads them from the session's buffer)"""
        dec = self.dec
        self._refill_cross(enc)
        self.seqs.fill_(dec.pad_token_id)
        self.seqs[:, 0] = dec.bos_token_id
        self.words.fill_(dec.bos_token_id)
        self.unfinished.fill_(1)
        self.pos.zero_()
        self.ticket.zero_()
        self.n_done.zero_()
        if self.tok_logp is not None:
            self.tok_logp.zero_()
        if self.uniforms is not None:
            if uniforms is not None:
                self.uniforms.copy_(uniforms)
            else:
                torch.rand(self.uniforms.shape, generator=generator, dtype=F32, device=self.uniforms.device, out=self.uniforms)

    def _run_iter(self, enc, return_logprobs=False, return_scores=False, step_hook=None, burst=0, uniforms=None, generator=None):
        """-> packed (B * n, max_len + 1) int64: ids padded with [PAD], the last column the row's length in columns ([BOS] and [EOS]
        included; unpack() trims) [, tok_logp (B * n, max_len) f32] [, scores (B * n,) f64 = sum of the chosen tokens' log-probabilities /
        generated length].  Yields as _GPT2Session._run_iter does."""
        max_len, eos = self.max_len, self.dec.eos_token_id
        hook = step_hook if step_hook is not None else (lambda *a: None)
        self._refill(enc, uniforms, generator)
        self._trunk()                                                    # position 0: every row reads [BOS]
        hook(0, self.logp_buf, None)
        # body number i chooses column i + 1 from the logits of position i and writes those of position i + 1
        yield from self._drive(max_len - 2, 1, step_hook, burst, (None,), stop=self._stopper())
        self._book(True)                                                 # the last column: nothing follows it
        decode._reap_plans()
        decode.stats['gpt2_steps_issued'] = self.issued + 1
        decode.stats['gpt2_route'] = 'sample'
        ended = self.seqs[:, 1:] == eos
        lens = torch.where(ended.any(1), ended.int().argmax(1) + 2, torch.full_like(self.seqs[:, 0], max_len))
        out = [torch.cat([self.seqs, lens.view(-1, 1)], dim=1)]
        if return_logprobs:
            out.append(self.tok_logp.clone())
        if return_scores:
            out.append(self.tok_logp.double().sum(1) / (lens - 1).double())
        return out[0] if len(out) == 1 else tuple(out)


def unpack(packed, host=None):
    """the session's packed result -> (B * n, L) ids with L = min(longest, max_seq_len) (one read of the lengths on the host; `host`: a copy
    of `packed` that is already there)"""
    lens = (host if host is not None else packed)[:, -1]
    L = min(int(lens.max()), packed.shape[1] - 1)
    return packed[:, :L]


def search(dec, enc, n_return, return_scores=False, step_hook=None, slot=0, as_iterator=False, burst=0, nb=None, opts=None):
    """the device route of DistilGPT2TextDecoderModel.generate at width nb (default: the decoder's beam_size); opts: the beam options
    resolved and validated by generate (keys of BEAM_NEUTRAL) -- None or all neutral: the plain beam session; as_iterator: a generator that
    yields after every issued step and returns the PACKED result (see _run_iter / unpack)"""
    B, S, dev = enc.shape[0], enc.shape[1], enc.device
    nb, max_len = int(dec.beam_size if nb is None else nb), int(dec.max_seq_len)
    if opts is None or dict(opts) == BEAM_NEUTRAL:
        key = ('gpt2', B, nb, max_len, S, dev.index, slot, n_return)
        ses = decode._session_for(dec, key, lambda: _GPT2Session(dec, B, nb, max_len, S, dev, slot, n_return))
    else:
        key = ('gpt2-beam-options', B, nb, max_len, S, dev.index, slot, n_return, tuple(sorted(opts.items())))
        ses = decode._session_for(dec, key, lambda: _GPT2BeamOptionsSession(dec, B, nb, max_len, S, dev, opts, slot, n_return))
    enc = enc.contiguous()
    if as_iterator:
        return ses.run_iter(enc, return_scores, step_hook, burst)
    out = ses.run(enc, return_scores, step_hook)
    if return_scores:
        return unpack(out[0]).contiguous(), out[1]
    return unpack(out).contiguous()


def sample(dec, enc, n, opts, return_logprobs=False, return_scores=False, step_hook=None, uniforms=None, generator=None, slot=0,
           as_iterator=False, burst=0):
    """the sampling / processor route of DistilGPT2TextDecoderModel.generate (opts: the controls resolved and validated by generate);
    as_iterator: a generator that yields after every issued step and returns the PACKED result (see _GPT2SampleSession._run_iter)"""
    B, S, dev = enc.shape[0], enc.shape[1], enc.device
    max_len = int(dec.max_seq_len)
    with_logp = bool(return_logprobs or return_scores)
    key = ('gpt2-sample', B, n, max_len, S, dev.index, slot, tuple(sorted(opts.items())), with_logp)
    ses = decode._session_for(dec, key, lambda: _GPT2SampleSession(dec, B, n, max_len, S, dev, opts, with_logp, slot))
    enc = enc.contiguous()
    if as_iterator:
        return ses.run_iter(enc, return_logprobs, return_scores, step_hook, burst, uniforms, generator)
    out = ses.run(enc, return_logprobs, return_scores, step_hook, 0, uniforms, generator)
    if not isinstance(out, tuple):
        return unpack(out).contiguous()
    L = unpack(out[0]).shape[1]
    return (out[0][:, :L].contiguous(),) + tuple(o[:, :L].contiguous() if o.dim() == 2 else o for o in out[1:])
