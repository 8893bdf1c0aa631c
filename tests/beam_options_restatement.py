"""CPU restatement (test infrastructure) of beam search with the reference's working option set (group_size 1):
CaptionModel.beam_search / beam_step (modules/caption_model.py:51-202) with temperature, decoding_constraint and length_penalty
(modules/utils.py:160-186), and AttModel._sample_beam's output for sample_n = 1 and sample_n = beam_size (modules/att_model.py:98-137),
over any `step(words, t, parent_rows) -> logp` callable:
    step(None, 0, None)          -> (B, V1) f32 log-probabilities of position 0 (one row per study),
    step(words, t, parent_rows)  -> (B * beam, V1) f32 log-probabilities of position t >= 1, BEFORE the temperature; words (B * beam,) are
                                    the words of position t - 1 in the new hypothesis order and parent_rows (B * beam,) the row each
                                    hypothesis had at the previous call (the reference's state_ix).
Everything that is stored is float32 like the reference's; the penalty and the ranking run in Python floats (the reference reads `p` with
.item()).  tests/test_beam_options_cpu.py pins this file to the reference through tests/golden/beam_options_stub.npz.
"""
import numpy as np
import torch
import torch.nn.functional as F


def parse_length_penalty(cfg):
    """utils.penalty_builder's reading -> ('', 0.0) | ('avg', alpha) | ('wu', alpha); anything else is a ValueError (the reference returns
    None there and fails at the first finished beam)"""
    if cfg == '':
        return '', 0.0
    parts = cfg.split('_')
    if len(parts) != 2 or parts[0] not in ('wu', 'avg'):
        raise ValueError('length_penalty %r' % (cfg,))
    return parts[0], float(parts[1])


def penalise(kind, alpha, length, p):
    """utils.length_wu / length_average on Python floats"""
    if kind == '':
        return p
    if kind == 'avg':
        return p / length
    return p / (((5 + length) ** alpha) / ((5 + 1) ** alpha))


def length_divisors(cfg, max_len):
    """the modifier of every length 1 .. max_len as float64 (what the engine hands to evk_beam_step_opts), None for ''"""
    kind, alpha = parse_length_penalty(cfg)
    if kind == '':
        return None
    return np.array([float(t) if kind == 'avg' else ((5 + t) ** alpha) / ((5 + 1) ** alpha) for t in range(1, max_len + 1)], dtype=np.float64)


def beam_search(step, B, beam, max_len, eos, opts=None, n_near=4):
    """-> dict(done = per study the finished list after the stable descending sort, cut to `beam`: dicts with seq (len,) int64, p (float,
    penalised), len, logps (len, V1) f32, rows (len,) = the row of each position's call that scored it; margin (max_len, B) = score of the
    last selected minus the first rejected candidate per step; trace = per step the `beam + n_near` best candidates (flat index, score, log-probability);
    rank_gap (B, beam) = list score k minus list score k + 1 over ALL finished hypotheses (inf where nothing follows); live_seq / live_sum /
    live_rows = the hypotheses, their running sums (after the -1000 of finished ones) and row ancestry as the last step left them)"""
    opts = opts or {}
    temperature = float(opts.get('temperature', 1.0))
    constraint = int(opts.get('decoding_constraint', 0))
    kind, alpha = parse_length_penalty(opts.get('length_penalty', ''))
    logprobs = step(None, 0, None).float().clone()
    V1 = logprobs.shape[-1]
    beam_seq = torch.zeros(B, beam, 0, dtype=torch.long)
    beam_lp = torch.zeros(B, beam, 0, V1)
    beam_rows = torch.zeros(B, beam, 0, dtype=torch.long)
    beam_sum = torch.zeros(B, beam)
    done = [[] for _ in range(B)]
    margin, trace = [], []
    for t in range(max_len):
        if constraint and t > 0:
            logprobs.scatter_(1, beam_seq[:, :, t - 1].reshape(-1, 1), float('-inf'))
        lp = logprobs.reshape(B, -1, V1)
        nb = lp.shape[1]
        cand = (beam_sum[:, :nb].unsqueeze(-1) + lp).reshape(B, -1)
        srt, ix = torch.sort(cand, -1, True)
        k = min(beam + n_near, cand.shape[1])
        trace.append(dict(flat=ix[:, :k].clone(), score=srt[:, :k].clone(), logp=lp.reshape(B, -1).gather(1, ix[:, :k]), n_beams=nb))
        margin.append((srt[:, beam - 1] - srt[:, beam]).numpy() if cand.shape[1] > beam else np.full(B, np.inf, dtype=np.float32))
        ix = ix[:, :beam]
        beam_ix, word_ix = ix // V1, ix % V1
        state_ix = (beam_ix + torch.arange(B).unsqueeze(-1) * nb).reshape(-1)
        if t > 0:
            beam_seq = beam_seq.gather(1, beam_ix.unsqueeze(-1).expand_as(beam_seq))
            beam_lp = beam_lp.gather(1, beam_ix.unsqueeze(-1).unsqueeze(-1).expand_as(beam_lp))
            beam_rows = beam_rows.gather(1, beam_ix.unsqueeze(-1).expand_as(beam_rows))
        beam_seq = torch.cat([beam_seq, word_ix.unsqueeze(-1)], -1)
        beam_sum = beam_sum[:, :nb].gather(1, beam_ix) + lp.reshape(B, -1).gather(1, ix)
        beam_lp = torch.cat([beam_lp, logprobs[state_ix].reshape(B, beam, 1, V1)], 2)
        beam_rows = torch.cat([beam_rows, state_ix.reshape(B, beam, 1)], 2)
        for b in range(B):
            is_end = beam_seq[b, :, t] == eos
            if t == max_len - 1:
                is_end = torch.ones_like(is_end)
            for vix in range(beam):
                if is_end[vix]:
                    done[b].append(dict(seq=beam_seq[b, vix].clone(), logps=beam_lp[b, vix].clone(), rows=beam_rows[b, vix].clone(), len=t + 1,
                                        p=penalise(kind, alpha, t + 1, beam_sum[b, vix].item())))
            beam_sum[b, is_end] -= 1000
        if t == max_len - 1:
            break
        raw = step(beam_seq[:, :, t].reshape(-1), t + 1, state_ix).float()
        logprobs = F.log_softmax(raw / temperature, dim=-1)
    rank_gap = np.full((B, beam), np.inf)
    for b in range(B):
        every = sorted(done[b], key=lambda x: -x['p'])
        for k in range(min(beam, len(every) - 1)):
            rank_gap[b, k] = every[k]['p'] - every[k + 1]['p']
        done[b] = every[:beam]
    return dict(done=done, margin=np.stack(margin), trace=trace, rank_gap=rank_gap, live_seq=beam_seq, live_sum=beam_sum, live_rows=beam_rows)


def output(res, B, beam, max_len, sample_n, pad=0):
    """AttModel._sample_beam's return values from beam_search()'s lists -> (seq (rows, max_len) int64, seq_logprobs (rows, max_len, V1) f32,
    scores (rows,) f64, lens (rows,))"""
    if sample_n not in (1, beam):
        raise ValueError('sample_n must be 1 or beam_size')
    V1 = res['done'][0][0]['logps'].shape[-1]
    rows = B * sample_n
    seq = torch.full((rows, max_len), pad, dtype=torch.long)
    slp = torch.zeros(rows, max_len, V1)
    scores, lens = np.zeros(rows), np.zeros(rows, dtype=np.int64)
    for b in range(B):
        for k in range(sample_n):
            e, r = res['done'][b][k], b * sample_n + k
            seq[r, :e['len']] = e['seq']
            slp[r, :e['len']] = e['logps']
            scores[r], lens[r] = e['p'], e['len']
    return seq, slp, scores, lens


def table_step(table, start_words):
    """the table-driven stub of tests/golden/make_golden_beam_options.py: log-probabilities are a fixed function of position and last
    word, table (max_len, V1, V1) f32, position 0 reads the row of each study's start word"""
    table = torch.as_tensor(table)
    start_words = torch.as_tensor(start_words, dtype=torch.long)

    def step(words, t, parent_rows):
        return table[t][start_words if words is None else words].clone()
    return step


def model_step(P, enc_states, enc_mask, cfg, bos, beam):
    """the oracle's decoder (oracle.beam._step_logprobs: the whole prefix is re-decoded every step, as the reference does)"""
    from oracle import beam as OB, functional as O
    ctx = O.Ctx()
    att, am = enc_states[:, 1:, :], enc_mask[:, 1:]
    B = att.shape[0]
    src_mask = am.unsqueeze(-2)
    memory = O.r2_encode(P, O.r2_att_embed(P, att, am, ctx), src_mask, ctx, cfg)
    memory_r = memory.unsqueeze(1).expand(-1, beam, -1, -1).reshape(B * beam, *memory.shape[1:])
    mask_r = src_mask.unsqueeze(1).expand(-1, beam, -1, -1).reshape(B * beam, *src_mask.shape[1:])
    state = {'ys': torch.full((B, 1), bos, dtype=torch.long)}

    def step(words, t, parent_rows):
        if words is None:
            return OB._step_logprobs(P, state['ys'], memory, src_mask, cfg, ctx)
        state['ys'] = torch.cat([state['ys'][parent_rows], words.reshape(-1, 1)], dim=1)
        return OB._step_logprobs(P, state['ys'], memory_r, mask_r, cfg, ctx)
    return step
