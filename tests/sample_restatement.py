"""CPU restatement (test infrastructure) of the sampling decode route: AttModel._sample's per-position bookkeeping
(modules/att_model.py:176-221: decoding constraint, trigram blocking, stored log-probability rows, finished rows) and
CaptionModel.sample_next_word's filtering (modules/caption_model.py:363-401: temperature, top-k, nucleus), on top of the oracle's
decoder step (oracle.beam._step_logprobs).  The categorical draw is restated as an inverse CDF over the kept entries in vocabulary order
with a supplied uniform number, which is how the engine draws (the reference asks torch.distributions for a sample: same distribution,
another generator).  The filter and the CDF are computed sequentially in float64; everything that is stored is float32 like the reference's.
"""
import numpy as np
import torch

from oracle import beam as OB, functional as O

GREEDY, SAMPLE, TOPK, TOPP = 0, 1, 2, 3        # the method codes of evk_sample_step


def parse_method(sample_method):
    """sample_next_word's reading of `sample_method` -> (code, parameter)"""
    if sample_method == 'greedy':
        return GREEDY, 0.0
    if sample_method == 'gumbel':
        raise NotImplementedError('gumbel')
    if sample_method.startswith('top'):
        top_num = float(sample_method[3:])
        if 0 < top_num < 1:
            return TOPP, top_num
        return TOPK, float(int(top_num))
    return SAMPLE, 0.0


def adjust_rows(logp, seq, t, block_rows, decoding_constraint):
    """logp (R, V1) f32 of position t, seq (R, >= t) the words so far -> the rows after the constraint and the trigram penalty (f32, new tensor)"""
    logp = logp.clone()
    R = logp.shape[0]
    if decoding_constraint and t > 0:
        tmp = torch.zeros_like(logp)
        tmp.scatter_(1, seq[:, t - 1].unsqueeze(1), float('-inf'))
        logp = logp + tmp
    if block_rows > 0 and t >= 3:
        mask = torch.zeros_like(logp)
        for r in range(min(block_rows, R)):
            h = seq[r, :t].tolist()
            a, b = h[t - 2], h[t - 1]
            for k in range(2, t):
                if h[k - 2] == a and h[k - 1] == b:
                    mask[r, h[k]] += 1                     # counts, not flags
        logp = logp + (mask * -0.693 * 2.0)
    return logp


def filter_row(row, temperature, method, param):
    """row (V1,) f32 after adjust_rows -> dict(weights f64 (V1,) of the kept entries (0 elsewhere, unnormalised), kept bool (V1,),
    gap = distance of the filter's decision from its boundary: top-k the k-th minus the (k+1)-th value, top-p the smallest
    |cumulative probability - p| over the descending order)"""
    y = row.double().numpy() / float(temperature)
    prob = np.exp(y - y.max())
    prob = prob / prob.sum()
    order = np.argsort(-y, kind='stable')              # descending, ties to the lower index
    kept = np.zeros(y.shape[0], dtype=bool)
    gap = np.inf
    if method == SAMPLE:
        kept[:] = True
    elif method == TOPK:
        k = int(param)
        kept[order[:k]] = True
        if k < y.shape[0]:
            d = y[order[k - 1]] - y[order[k]]
            gap = np.inf if np.isnan(d) else d
    elif method == TOPP:
        before = 0.0
        for i in order:                                # sequential cumulative sum, as torch.cumsum over the sorted row
            if before < param or i == order[0]:
                kept[i] = True
            gap = min(gap, abs(before - param)) if i != order[0] else gap
            before += prob[i]
    else:
        raise ValueError(method)
    return dict(weights=np.where(kept, prob, 0.0), kept=kept, gap=gap)


def draw(weights, u):
    """inverse CDF in vocabulary order: the first w whose running sum exceeds u * total -> (w, distance of u from the nearest CDF step)"""
    cdf = np.cumsum(weights) / weights.sum()
    w = int(np.searchsorted(cdf, u, side='right'))
    if w >= len(cdf):
        w = int(np.nonzero(weights > 0)[0][-1])
    steps = cdf[weights > 0]
    return w, float(np.min(np.abs(steps - u)))


def sample_step(logp, seq, unfinished, t, eos, pad, block_rows, decoding_constraint, temperature, method, param, uniforms=None):
    """one position of _sample on (R, V1) log-probabilities.  seq (R, T) int64 and unfinished (R,) bool are updated IN PLACE as the
    reference does -> dict(words (R,) int64, stored (R, V1) f32 = the seqLogprobs row (zeros for a finished row), kept / filter_gap /
    draw_gap per row for the stochastic methods)"""
    R = logp.shape[0]
    rows = adjust_rows(logp, seq, t, block_rows, decoding_constraint)
    out = dict(kept=[None] * R, filter_gap=[np.inf] * R, draw_gap=[np.inf] * R)
    if method == GREEDY:
        it = torch.max(rows, 1).indices.long()
    else:
        it = torch.zeros(R, dtype=torch.long)
        for r in range(R):
            f = filter_row(rows[r], temperature, method, param)
            w, dg = draw(f['weights'], float(uniforms[r, t]))
            it[r] = w
            out['kept'][r], out['filter_gap'][r], out['draw_gap'][r] = f['kept'], f['gap'], dg
    if t == 0:
        unfinished[:] = it != eos
        stored = rows
    else:
        it[~unfinished] = pad
        # (logprobs * unfinished; the reference's -inf * 0 = NaN in the constrained column of a finished row is restated as 0)
        stored = torch.where(unfinished.unsqueeze(1), rows, torch.zeros_like(rows))
        unfinished &= it != eos
    seq[:, t] = it
    out.update(words=it.clone(), stored=stored)
    return out


def sample(P, enc_states, enc_mask, cfg, bos, eos, pad=0, ctx=None, uniforms=None):
    """AttModel._sample -> (seq (R, max_seq_len) int64 padded with `pad`, seq_logprobs (R, max_seq_len, V+1) f32), R = B * sample_n.
    cfg: max_seq_len, sample_method, sample_n, temperature, block_trigrams, decoding_constraint beside the oracle's own keys."""
    ctx = ctx or O.Ctx()
    max_len, n = int(cfg['max_seq_len']), int(cfg.get('sample_n', 1))
    method, param = parse_method(cfg.get('sample_method', 'greedy'))
    att, am = enc_states[:, 1:, :], enc_mask[:, 1:]
    B = att.shape[0]
    R = B * n
    src_mask = am.unsqueeze(-2)
    memory = O.r2_encode(P, O.r2_att_embed(P, att, am, ctx), src_mask, ctx, cfg)
    memory = memory.repeat_interleave(n, 0)              # utils.repeat_tensors: the copies of a study are neighbours
    src_mask = src_mask.repeat_interleave(n, 0)
    ys = torch.full((R, 1), bos, dtype=torch.long)
    seq = torch.full((R, max_len), pad, dtype=torch.long)
    unfinished = torch.ones(R, dtype=torch.bool)
    seq_logprobs = None
    for t in range(max_len):
        logp = OB._step_logprobs(P, ys, memory, src_mask, cfg, ctx)
        if seq_logprobs is None:
            seq_logprobs = torch.zeros(R, max_len, logp.shape[1])
        # `for i in range(batch_size)` over the repeated rows: only the first B of the R rows are blocked
        st = sample_step(logp, seq, unfinished, t, eos, pad, B if cfg.get('block_trigrams', 0) else 0, cfg.get('decoding_constraint', 0),
                         cfg.get('temperature', 1.0), method, param, uniforms)
        seq_logprobs[:, t] = st['stored']
        if not unfinished.any():
            break
        ys = torch.cat([ys, st['words'].unsqueeze(1)], 1)
    return seq, seq_logprobs


def digest(seq, logp, probe_ids, n_top=8):
    """the arrays a fixture of tests/golden/make_sample_golden.py holds, from this side's results"""
    lp = logp.float()
    order = torch.sort(-lp, dim=-1, stable=True).indices[..., :n_top]
    top = lp.gather(-1, order)
    return dict(seq=seq.numpy(), top_ids=order.numpy(), top_logp=top.numpy(), probe_logp=lp[..., probe_ids].numpy(),
                margin=(top[..., 0] - top[..., 1]).numpy())
