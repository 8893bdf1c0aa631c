"""distilgpt2 cross-attention decoder backend on the HIP engine -- mirror of DistilGPT2TextDecoderModel
(models/language_encoder/language_model.py:161-282).

The reference class wraps HF GPT2LMHeadModel(add_cross_attention=True) in an EncoderDecoderModel with a dummy encoder; its
state_dict keys are `decoder.encoder_decoder.decoder.{transformer.{wte,wpe,h.<i>.*,ln_f},lm_head}.*` (HF Conv1D weights are
(in, out)).  Same constructor `(config, tokenizer)`, same `forward(encoder_hidden_states, encoder_attention_mask,
input_ids, attention_mask, stage)`; `stage='train'` returns the un-shifted cross-entropy of lines 252-254, `stage='test'`
HF-style beam search (2*num_beams candidates, length-normalised finished hypotheses) with K/V caches; generate() also serves HF's
sampling / greedy decoding with logits processors (num_beams 1) and beam search with the repetition_penalty / no_repeat_ngram_size /
min_length processors, length_penalty, early_stopping and an explicit num_beams (configuration keys num_beams, early_stopping,
gpt2_length_penalty).
Selected in FineTune by args['text_decoder'] = 'distilgpt2' (the key exists only as a comment in modules/utils.py:78)."""
import math

import torch
import torch.nn as nn

from . import hip as H
from . import ops
from .layers import EmbP, LayerNormP
from .ops import BF16, F32


class Conv1DP(nn.Module):
    """transformers.pytorch_utils.Conv1D parameter holder: weight (in, out), bias (out)."""

    def __init__(self, nf, nx):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(nx, nf) * 0.02)
        self.bias = nn.Parameter(torch.zeros(nf))

    def forward(self, x, resid=None):
        return ops.linear_t(x, self.weight, self.bias, resid=resid)


class _Attn(nn.Module):
    def __init__(self, d, cross):
        super().__init__()
        if cross:
            self.c_attn = Conv1DP(2 * d, d)
            self.q_attn = Conv1DP(d, d)
        else:
            self.c_attn = Conv1DP(3 * d, d)
        self.c_proj = Conv1DP(d, d)


class _MLP(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.c_fc = Conv1DP(4 * d, d)
        self.c_proj = Conv1DP(d, 4 * d)


class GPT2Block(nn.Module):
    def __init__(self, d, heads, eps=1e-5, p_attn=0.1, p_resid=0.1):
        super().__init__()
        self.ln_1 = LayerNormP(d, eps)
        self.attn = _Attn(d, False)
        self.ln_2 = LayerNormP(d, eps)
        self.crossattention = _Attn(d, True)
        self.ln_cross_attn = LayerNormP(d, eps)
        self.mlp = _MLP(d)
        self.d, self.heads, self.p_attn, self.p_resid = d, heads, p_attn, p_resid

    def _proj(self, conv, a, x):
        if self.training and self.p_resid > 0 and ops.DROPOUT_ENABLED[0]:
            return ops.dropout(conv(a), self.p_resid, True, resid=x)
        return conv(a, resid=x)

    def forward(self, x, enc, key_mask, cache=None, pos=None):
        d, tr = self.d, self.training
        q, k, v = [t.contiguous() for t in self.attn.c_attn(self.ln_1(x)).split(d, dim=2)]
        if cache is not None:                                    # incremental decode: append to the K/V cache
            cache['k'][:, pos:pos + 1], cache['v'][:, pos:pos + 1] = k, v
            k, v = cache['k'][:, :pos + 1].contiguous(), cache['v'][:, :pos + 1].contiguous()
            a = ops.attention(q, k, v, self.heads)
        else:
            a = ops.attention(q, k, v, self.heads, mask=key_mask, causal=True, p_drop=self.p_attn, training=tr)
        x = self._proj(self.attn.c_proj, a, x)
        q = self.crossattention.q_attn(self.ln_cross_attn(x))
        if cache is not None and 'ck' in cache:
            ck, cv = cache['ck'], cache['cv']
        else:
            ck, cv = [t.contiguous() for t in self.crossattention.c_attn(enc).split(d, dim=2)]
            if cache is not None:
                cache['ck'], cache['cv'] = ck, cv
        a = ops.attention(q, ck, cv, self.heads, p_drop=self.p_attn, training=tr)
        x = self._proj(self.crossattention.c_proj, a, x)
        f = ops.activation(self.mlp.c_fc(self.ln_2(x)), H.ACT_GELU_NEW)
        return self._proj(self.mlp.c_proj, f, x)


class _Transformer(nn.Module):
    def __init__(self, vocab, d, layers, heads, n_pos):
        super().__init__()
        self.wte = EmbP(vocab, d)
        self.wpe = EmbP(n_pos, d)
        self.h = nn.ModuleList([GPT2Block(d, heads) for _ in range(layers)])
        self.ln_f = LayerNormP(d, 1e-5)


class _LMHead(nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = weight                      # tied to transformer.wte.weight (same Parameter object)


class _GPT2LMHead(nn.Module):
    def __init__(self, vocab, d, layers, heads, n_pos):
        super().__init__()
        self.transformer = _Transformer(vocab, d, layers, heads, n_pos)
        self.lm_head = _LMHead(self.transformer.wte.weight)


class _EncDec(nn.Module):
    def __init__(self, dec):
        super().__init__()
        self.decoder = dec


class _Holder(nn.Module):
    def __init__(self, dec):
        super().__init__()
        self.encoder_decoder = _EncDec(dec)


# Hugging Face's neutral values of the generate() controls this backend serves
_HF_NEUTRAL = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
# the beam controls of generate(): keyword -> configuration key (`length_penalty` itself is the R2Gen decoder's string form in the args)
_BEAM_KEYS = dict(num_beams='num_beams', length_penalty='gpt2_length_penalty', early_stopping='early_stopping')


class DistilGPT2TextDecoderModel(nn.Module):
    def __init__(self, config, tokenizer):
        super().__init__()
        d = config['decoder_hidden_size']
        self.vocab = config['vocab_size']
        self.heads = config.get('decoder_num_attention_heads', 12)
        self.layers = config['decoder_num_hidden_layers']
        self.decoder = _Holder(_GPT2LMHead(self.vocab, d, self.layers, self.heads, config.get('n_positions', 1024)))
        self.pad_token_id = tokenizer.token_to_id('[PAD]')
        self.eos_token_id = tokenizer.token_to_id('[EOS]')
        self.bos_token_id = tokenizer.token_to_id('[BOS]')
        self.beam_size = config['beam_size']
        self.max_seq_len = config['max_seq_len']
        self.sample_n = int(config.get('sample_n', 1))         # default of generate(num_return_sequences=...)
        # defaults of generate()'s Hugging Face controls: the keys of the same names, where the configuration carries them
        self.generation = {k: config[k] for k in _HF_NEUTRAL if config.get(k) is not None}
        self.beam_controls = {k: config[c] for k, c in _BEAM_KEYS.items() if config.get(c) is not None}
        self.generator = config.get('generator')
        self.p_embd = 0.1

    @property
    def gpt2(self):
        return self.decoder.encoder_decoder.decoder

    def _hidden(self, ids, attention_mask, enc, caches=None, pos=None):
        t = self.gpt2.transformer
        pe = t.wpe.weight if pos is None else t.wpe.weight[pos:pos + 1]
        x = ops.dropout(ops.embedding(ids.contiguous(), t.wte.weight, pos=pe), self.p_embd, self.training)
        km = attention_mask.to(torch.uint8).contiguous() if attention_mask is not None else None
        for i, blk in enumerate(t.h):
            x = blk(x, enc, km, None if caches is None else caches[i], pos)
        return t.ln_f(x)

    def logits(self, ids, attention_mask, enc, caches=None, pos=None):
        """f32 logits (B, L, pad8(V)) through the tied head."""
        return ops.linear(self._hidden(ids, attention_mask, enc, caches, pos), self.gpt2.lm_head.weight, None, out_f32=True)

    def forward(self, encoder_hidden_states, encoder_attention_mask, input_ids=None, attention_mask=None, stage='train'):
        assert stage in ['train', 'test']
        if stage == 'train':
            lg = self.logits(input_ids, attention_mask, encoder_hidden_states)
            w = (input_ids != self.pad_token_id).to(F32)
            return ops.nll_loss(lg, input_ids.reshape(-1), w.reshape(-1), self.vocab)
        return self.generate(encoder_hidden_states)

    def session_available(self, S=None):
        """generate() takes the device route (evoke_amd/gpt2_decode.py) for this decoder (and an encoder output of S positions)"""
        from .gpt2_decode import session_usable
        return session_usable(self, S)

    @torch.no_grad()
    def generate(self, enc, num_return_sequences=None, return_scores=False, step_hook=None, slot=0, as_iterator=False, burst=0, *,
                 do_sample=None, temperature=None, top_k=None, top_p=None, repetition_penalty=None, no_repeat_ngram_size=None,
                 min_length=None, uniforms=None, generator=None, return_logprobs=False, num_beams=None, length_penalty=None,
                 early_stopping=None):
        """HF beam search (num_beams = beam_size in 1..8, max_length = max_seq_len, length_penalty 1, early_stopping False) -> (B * n, L) ids
        starting with [BOS], padded with [PAD], L = min(longest, max_seq_len): the n = num_return_sequences (default: config sample_n, 1)
        best hypotheses of every study next to each other; with return_scores also their scores (B * n,) f64 = HF's sequences_scores.
        The search runs on the device (gpt2_decode: one captured step per token, no host synchronisation in the loop) whenever it can:
        head size 64 / 128 / 256, 5 <= max_seq_len <= 256, graph capture enabled, EVK_GPT2_SESSION not '0'.  Otherwise the host-driven
        loop (_generate_host), which serves beam_size <= 4 and n = 1 only and refuses the rest with NotImplementedError.
        step_hook(t, logp, scores): test instrument, called on the launching stream before the bookkeeping of position t reads `logp`
        (f32 (B * beam, V), may be edited in place); slot / as_iterator / burst: as decode.beam_search -- the iterator returns the packed
        result of gpt2_decode._GPT2Session._run_iter.
        Sampling and logits processors (Hugging Face's names, semantics and order; None: the configuration's key of that name, else HF's
        neutral value): do_sample (False), temperature (1.0), top_k (0), top_p (1.0), repetition_penalty (1.0), no_repeat_ngram_size (0,
        at most 8), min_length (0).  With do_sample, or with any of repetition_penalty / no_repeat_ngram_size / min_length switched on
        (temperature, top_k and top_p act only when do_sample, as in HF), the search is gpt2_decode._GPT2SampleSession: beam_size must
        be 1, num_return_sequences > 1 needs do_sample, there is no host-driven route (NotImplementedError where the device session does
        not serve the geometry).  -> (B * n, L) ids [, with return_logprobs (B * n, L) f32 log-probabilities of the chosen tokens under
        the processed distribution, column 0 = 0] [, with return_scores their per-row sum / generated length, f64].  uniforms: f32
        (B * n, max_seq_len) on enc's device, the numbers in [0, 1) of the inverse-CDF draws (column c draws the id of column c); absent:
        torch.rand on the device with `generator` (default: the configuration's `generator`, else the global one).
        step_hook(t, logits, None) on this route: before the choice at step t reads the f32 logits rows (B * n, V).
        Beam controls (None: the configuration's key, else the neutral value): num_beams (key num_beams; else beam_size), length_penalty
        (key gpt2_length_penalty; 1.0: a hypothesis score is its sum / cur_len ** length_penalty), early_stopping (key early_stopping; False;
        a bool -- "never" does not exist in the reference's pinned transformers).  While no num_beams is given and the other two are
        neutral, everything above holds unchanged.  Otherwise the search is a beam search of width num_beams (else beam_size) in 1..8 with
        num_return_sequences <= width, on which repetition_penalty, no_repeat_ngram_size and min_length act as in HF's beam mode -- on the
        log-probability rows of every running beam, from that beam's own history -- through gpt2_decode._GPT2BeamOptionsSession (the plain
        beam session at that width when every option is neutral).  There is no host-driven route for it (NotImplementedError where the
        device session does not serve the geometry; with graph capture disabled the steps are issued eagerly); do_sample (beam sampling)
        and return_logprobs are refused with NotImplementedError."""
        bc = self._beam_controls(num_beams, length_penalty, early_stopping)
        if bc is not None:
            return self._generate_beam_options(enc, bc, num_return_sequences, return_scores, return_logprobs, step_hook, slot, as_iterator, burst,
                                               uniforms, dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p,
                                                              repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                                              min_length=min_length))
        o = self._generation_options(do_sample, temperature, top_k, top_p, repetition_penalty, no_repeat_ngram_size, min_length)
        if o is not None:
            return self._generate_processed(enc, o, num_return_sequences, return_scores, return_logprobs, step_hook, slot, as_iterator, burst,
                                            uniforms, generator)
        if return_logprobs:
            raise NotImplementedError('return_logprobs needs do_sample or a logits processor (the beam search returns scores)')
        nb = int(self.beam_size)
        if not 1 <= nb <= 8:
            raise ValueError('beam_size must be in [1, 8] for the distilgpt2 backend, not %d' % nb)
        n = self.sample_n if num_return_sequences is None else int(num_return_sequences)
        if not 1 <= n <= nb:
            raise ValueError('num_return_sequences must be in [1, beam_size = %d], not %d' % (nb, n))
        if self.vocab < 2 * nb:
            raise ValueError('the vocabulary must hold 2 * beam_size candidates')
        if self.session_available(enc.shape[1]):
            from . import gpt2_decode
            return gpt2_decode.search(self, enc, n, return_scores, step_hook, slot, as_iterator, burst)
        if nb > 4 or n > 1 or return_scores or as_iterator or step_hook is not None:
            raise NotImplementedError('beam_size > 4, num_return_sequences > 1, scores, step hooks and stepwise iteration need the device '
                                      'route of the distilgpt2 search')
        return self._generate_host(enc)

    def _generation_options(self, do_sample, temperature, top_k, top_p, repetition_penalty, no_repeat_ngram_size, min_length):
        """the controls of generate() resolved against the configuration and checked -> dict (keys of _HF_NEUTRAL), or None when they leave
        the beam search as it is"""
        given = dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                     no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length)
        o = {k: (v if v is not None else self.generation.get(k, _HF_NEUTRAL[k])) for k, v in given.items()}
        o = dict(do_sample=bool(o['do_sample']), temperature=float(o['temperature']), top_k=int(o['top_k']), top_p=float(o['top_p']),
                 repetition_penalty=float(o['repetition_penalty']), no_repeat_ngram_size=int(o['no_repeat_ngram_size']),
                 min_length=int(o['min_length']))
        if not o['temperature'] > 0:
            raise ValueError('temperature must be > 0, not %r' % o['temperature'])
        if not 0 < o['top_p'] <= 1:
            raise ValueError('top_p must be in (0, 1], not %r' % o['top_p'])
        if o['top_k'] < 0:
            raise ValueError('top_k must be >= 0, not %r' % o['top_k'])
        if not o['repetition_penalty'] > 0:
            raise ValueError('repetition_penalty must be > 0, not %r' % o['repetition_penalty'])
        if not 0 <= o['no_repeat_ngram_size'] <= 8:
            raise ValueError('no_repeat_ngram_size must be in [0, 8], not %r' % o['no_repeat_ngram_size'])
        if o['min_length'] < 0:
            raise ValueError('min_length must be >= 0, not %r' % o['min_length'])
        if not o['do_sample']:
            # (the warpers act only on a sampling search, as in HF: a temperature the configuration carries for another route changes nothing)
            o.update(temperature=1.0, top_k=0, top_p=1.0)
        return None if o == _HF_NEUTRAL else o

    def _beam_controls(self, num_beams, length_penalty, early_stopping):
        """the beam controls of generate() resolved against the configuration and checked -> dict(num_beams = the width, length_penalty,
        early_stopping), or None when no num_beams is given and the scorer's controls are neutral (generate() then is what it was)"""
        given = dict(num_beams=num_beams, length_penalty=length_penalty, early_stopping=early_stopping)
        c = {k: (v if v is not None else self.beam_controls.get(k)) for k, v in given.items()}
        es = False if c['early_stopping'] is None else c['early_stopping']
        if isinstance(es, str):
            raise ValueError('early_stopping must be a bool: %r (and "never" in particular) does not exist in the pinned transformers 4.23.1' % es)
        if not isinstance(es, (bool, int)) or es not in (0, 1):
            raise ValueError('early_stopping must be a bool, not %r' % (es,))
        lp = 1.0 if c['length_penalty'] is None else c['length_penalty']
        if isinstance(lp, (str, bool)) or not math.isfinite(float(lp)):
            raise ValueError('length_penalty must be a finite number, not %r' % (lp,))
        lp, es = float(lp), bool(es)
        if c['num_beams'] is None and lp == 1.0 and not es:
            return None
        nb = int(self.beam_size if c['num_beams'] is None else c['num_beams'])
        if not 1 <= nb <= 8:
            raise ValueError('num_beams must be in [1, 8] for the distilgpt2 backend, not %d' % nb)
        return dict(num_beams=nb, length_penalty=lp, early_stopping=es)

    def _generate_beam_options(self, enc, bc, num_return_sequences, return_scores, return_logprobs, step_hook, slot, as_iterator, burst, uniforms,
                               controls):
        """generate() with a beam control given: the device beam search at width bc['num_beams'] with the processors and scorer controls"""
        o = self._generation_options(**controls) or dict(_HF_NEUTRAL)
        if o['do_sample']:
            raise NotImplementedError('do_sample with num_beams / length_penalty / early_stopping is beam sampling, which is not built '
                                      '(it differs between the pinned and later transformers releases)')
        if return_logprobs:
            raise NotImplementedError('return_logprobs is not built on the beam route (the beam search returns scores)')
        if uniforms is not None:
            raise ValueError('uniforms are the numbers of the draws: they need do_sample')
        nb = bc['num_beams']
        n = self.sample_n if num_return_sequences is None else int(num_return_sequences)
        if not 1 <= n <= nb:
            raise ValueError('num_return_sequences must be in [1, num_beams = %d], not %d' % (nb, n))
        if self.vocab < 2 * nb:
            raise ValueError('the vocabulary must hold 2 * num_beams candidates')
        from . import gpt2_decode
        if not gpt2_decode.session_usable(self, enc.shape[1], need_graph=False):
            raise NotImplementedError('num_beams, length_penalty, early_stopping and logits processors on a beam search need the device route '
                                      'of the distilgpt2 search: there is no host-driven route for them')
        opts = dict(repetition_penalty=o['repetition_penalty'], no_repeat_ngram_size=o['no_repeat_ngram_size'], min_length=o['min_length'],
                    length_penalty=bc['length_penalty'], early_stopping=bc['early_stopping'])
        return gpt2_decode.search(self, enc, n, return_scores, step_hook, slot, as_iterator, burst, nb=nb, opts=opts)

    def _generate_processed(self, enc, o, num_return_sequences, return_scores, return_logprobs, step_hook, slot, as_iterator, burst, uniforms,
                            generator):
        """generate() with do_sample or a logits processor switched on: the device session of gpt2_decode.sample"""
        if int(self.beam_size) != 1:
            raise NotImplementedError('sampling and logits processors need beam_size 1, not %d (a beam search takes repetition_penalty, '
                                      'no_repeat_ngram_size and min_length once num_beams is given)' % int(self.beam_size))
        n = self.sample_n if num_return_sequences is None else int(num_return_sequences)
        if n < 1 or (n > 1 and not o['do_sample']):
            raise ValueError('num_return_sequences must be >= 1, and 1 without do_sample, not %d' % n)
        R, max_len = enc.shape[0] * n, int(self.max_seq_len)
        if uniforms is not None:
            if not o['do_sample']:
                raise ValueError('uniforms are the numbers of the draws: they need do_sample')
            if (not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (R, max_len) or uniforms.dtype != torch.float32 or
                    uniforms.device != enc.device):
                raise ValueError('uniforms must be float32 %s on %s, not %s %s on %s'
                                 % ((R, max_len), enc.device, getattr(uniforms, 'dtype', type(uniforms)),
                                    tuple(getattr(uniforms, 'shape', ())), getattr(uniforms, 'device', None)))
        from . import gpt2_decode
        if not gpt2_decode.session_usable(self, enc.shape[1], need_graph=False):
            raise NotImplementedError('sampling and logits processors need the device route of the distilgpt2 search')
        if self.vocab > 12288:
            raise NotImplementedError('sampling and logits processors serve vocabularies up to 12288 entries, not %d' % self.vocab)
        return gpt2_decode.sample(self, enc, n, o, return_logprobs, return_scores, step_hook, uniforms,
                                  generator if generator is not None else self.generator, slot, as_iterator, burst)

    @torch.no_grad()
    def _generate_host(self, enc):
        """the search driven from the host (two device -> host copies per token): the route of geometries the device session does not serve"""
        was_training = self.training
        self.eval()
        try:
            nb, max_len, V = self.beam_size, self.max_seq_len, self.vocab
            if 2 * nb > 8:
                raise NotImplementedError('the host-driven search serves beam_size <= 4')
            B, dev, d = enc.shape[0], enc.device, enc.shape[-1]
            encx = enc.repeat_interleave(nb, dim=0).contiguous()
            R = B * nb
            caches = [dict(k=torch.zeros(R, max_len, d, dtype=BF16, device=dev), v=torch.zeros(R, max_len, d, dtype=BF16, device=dev))
                      for _ in range(self.layers)]
            seqs = torch.full((R, 1), self.bos_token_id, dtype=torch.long, device=dev)
            scores = torch.zeros(B, nb, dtype=F32, device=dev)
            scores[:, 1:] = -1e9
            scores = scores.view(-1)
            hyps = [[] for _ in range(B)]
            done = [False] * B
            cur_len = 1
            while cur_len < max_len:
                lg = self.logits(seqs[:, -1:].contiguous(), None, encx, caches, cur_len - 1)
                lp = ops.log_softmax(lg.view(R, -1), V) + scores[:, None]
                top_s, top_i = torch.empty(B, 2 * nb, dtype=F32, device=dev), torch.empty(B, 2 * nb, dtype=torch.long, device=dev)
                H.check(H.lib.evk_topk_rows(H.ptr(lp.view(B, nb * V).contiguous()), H.ptr(top_s), H.ptr(top_i), B, nb * V, 2 * nb, H.stream()))
                ts, ti = top_s.cpu(), top_i.cpu()
                nxt_scores = torch.zeros(B, nb)
                nxt_tok = torch.zeros(B, nb, dtype=torch.long)
                nxt_idx = torch.zeros(B, nb, dtype=torch.long)
                seq_cpu = None
                for b in range(B):
                    if done[b]:
                        nxt_tok[b] = self.pad_token_id
                        nxt_idx[b] = b * nb
                        continue
                    k = 0
                    for rank in range(2 * nb):
                        tok, bi, sc = int(ti[b, rank]) % V, int(ti[b, rank]) // V, float(ts[b, rank])
                        if tok == self.eos_token_id:
                            if rank >= nb:
                                continue
                            if seq_cpu is None:
                                seq_cpu = seqs.cpu()
                            hyps[b].append((sc / cur_len, torch.cat([seq_cpu[b * nb + bi], torch.tensor([tok])])))
                            hyps[b] = sorted(hyps[b], key=lambda x: -x[0])[:nb]
                        else:
                            nxt_scores[b, k], nxt_tok[b, k], nxt_idx[b, k] = sc, tok, b * nb + bi
                            k += 1
                        if k == nb:
                            break
                    if len(hyps[b]) >= nb and hyps[b][-1][0] >= float(ts[b].max()) / cur_len:
                        done[b] = True
                idx = nxt_idx.view(-1).to(dev)
                seqs = torch.cat([seqs.index_select(0, idx), nxt_tok.view(-1, 1).to(dev)], dim=1)
                scores = nxt_scores.view(-1).to(dev)
                for c in caches:
                    c['k'][:, :cur_len] = c['k'][:, :cur_len].index_select(0, idx)
                    c['v'][:, :cur_len] = c['v'][:, :cur_len].index_select(0, idx)
                cur_len += 1
                if all(done):
                    break
            seq_cpu, sc_cpu = seqs.cpu(), scores.cpu()
            out = []
            for b in range(B):
                if not done[b]:
                    for k in range(nb):
                        hyps[b].append((float(sc_cpu[b * nb + k]) / (cur_len - 1), seq_cpu[b * nb + k]))
                out.append(sorted(hyps[b], key=lambda x: -x[0])[0][1])
            L = min(max(len(o) for o in out), max_len)
            res = torch.full((B, L), self.pad_token_id, dtype=torch.long)
            for b, o in enumerate(out):
                res[b, :min(len(o), L)] = o[:L]
            return res.to(dev)
        finally:
            self.train(was_training)
