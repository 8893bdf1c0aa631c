"""CPU restatement (test infrastructure) of Hugging Face's sampling / greedy decoding with its standard logits processors, in the state
layout of evk_hf_sample_step (csrc/hf_sample.hip), so that a GPU test can compare after every token.  In HF's order, on the raw f32 logits:
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor, then with do_sample TemperatureLogitsWarper,
TopKLogitsWarper, TopPLogitsWarper.  What is stored is float32 like HF's; the filters' decisions, their distances from the boundary and the
CDF are computed in float64.  The categorical draw is restated as an inverse CDF over the kept entries in vocabulary order with a supplied
uniform number, which is how the engine draws (HF asks torch.multinomial: same distribution, another random stream).  Pure torch / Python."""
import numpy as np
import torch

NEUTRAL = dict(do_sample=False, temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0)
NEG_INF = float('-inf')


def options(**kw):
    bad = set(kw) - set(NEUTRAL)
    assert not bad, bad
    return dict(NEUTRAL, **kw)


def banned_ngram_ids(hist, g):
    """ids that would complete an n-gram of size g already present in hist (a list of ids, cur_len = len(hist))"""
    cur = len(hist)
    if g <= 0 or cur < g:
        return []
    tail = hist[cur - (g - 1):] if g > 1 else []
    return sorted({hist[i + g - 1] for i in range(cur - g + 1) if hist[i:i + g - 1] == tail})


def process_row(x, hist, eos, opts):
    """x (V,) f32 raw logits, hist: the ids so far ([BOS] included) -> dict(row (V,) f32 after every processor that applies,
    gap = distance of the closest filter decision from its boundary: top-k the k-th minus the (k+1)-th value, top-p the smallest
    |mass - (1 - p)| over the candidate boundaries, greedy the arg-max margin)"""
    x = x.clone().float()
    V, cur = x.shape[0], len(hist)
    rp = float(opts['repetition_penalty'])
    if rp != 1.0:
        ids = torch.tensor(sorted(set(h for h in hist if 0 <= h < V)), dtype=torch.long)
        v = x[ids]
        x[ids] = torch.where(v < 0, v * rp, v / rp)                      # f32 arithmetic, as HF
    for w in banned_ngram_ids(list(hist), int(opts['no_repeat_ngram_size'])):
        if 0 <= w < V:
            x[w] = NEG_INF
    if cur < int(opts['min_length']):
        x[eos] = NEG_INF
    gap = np.inf
    if not opts['do_sample']:
        top = torch.topk(x, 2).values.double()
        if torch.isfinite(top[0]):
            gap = float(top[0] - top[1])
        return dict(row=x, gap=gap)
    if float(opts['temperature']) != 1.0:
        x = x / float(opts['temperature'])                               # a division in f32, as HF
    k = min(int(opts['top_k']), V)
    if 0 < k < V:
        top = torch.topk(x, k + 1).values
        kth = top[k - 1]
        d = float(kth.double() - top[k].double())
        if d > 0:                                                        # (a tie at the boundary stays as a whole: no decision to miss)
            gap = min(gap, d)
        x = torch.where(x < kth, torch.full_like(x, NEG_INF), x)
    p = float(opts['top_p'])
    if p < 1.0 and bool(torch.isfinite(x).any()):
        y = x.double().numpy()
        prob = np.exp(y - y.max())
        prob = prob / prob.sum()
        order = np.argsort(y, kind='stable')                             # ascending
        cum = np.cumsum(prob[order])
        ends = np.searchsorted(y[order], y, side='right') - 1            # the last entry of the group of equal values
        mass = cum[ends]
        keep = mass > 1.0 - p
        keep[int(np.argmax(y))] = True
        keep |= y == y.max()
        live = np.isfinite(y) & (y < y.max())                            # (the maximum always stays: no decision there)
        if live.any():
            gap = min(gap, float(np.min(np.abs(mass[live] - (1.0 - p)))))
        x = torch.where(torch.from_numpy(keep), x, torch.full_like(x, NEG_INF))
    return dict(row=x, gap=gap)


def weights(row):
    """unnormalised f64 softmax weights of a processed row (0 for removed entries)"""
    y = row.double().numpy()
    if not np.isfinite(y).any():
        return np.zeros_like(y)
    return np.where(np.isfinite(y), np.exp(y - y[np.isfinite(y)].max()), 0.0)


def draw(w, u):
    """inverse CDF in vocabulary order: the first kept id whose running weight exceeds u * total -> (id, distance of u from the nearest CDF
    step)"""
    cdf = np.cumsum(w) / w.sum()
    kept = np.nonzero(w > 0)[0]
    steps = cdf[kept]
    j = int(np.searchsorted(steps, u, side='right'))
    tok = int(kept[min(j, len(kept) - 1)])
    return tok, float(np.min(np.abs(steps - u)))


def choose(row, do_sample, u, pad):
    """-> (id, log-probability of the id under the processed row (f32 value), distance of u from the nearest CDF step)"""
    w = weights(row)
    if w.sum() == 0:
        return pad, 0.0, np.inf
    if do_sample:
        tok, dg = draw(w, float(u))
    else:
        tok, dg = int(torch.argmax(row)), np.inf                        # ties: the lowest id
    lse = float(torch.logsumexp(row.double(), 0))
    return tok, float(np.float32(float(row[tok].double()) - lse)), dg


def step(logits, seqs, unfinished, cur_len, eos, pad, opts, uniforms=None):
    """one launch of evk_hf_sample_step with *pos = cur_len - 1: logits (R, V) f32; seqs (R, max_len) int64 and unfinished (R,) bool are
    updated IN PLACE -> dict(words (R,), rows (R, V) f32 processed, tok_logp (R,) f32, filter_gap / draw_gap per row, n_done = rows that
    finished in this step)"""
    R = logits.shape[0]
    words = torch.zeros(R, dtype=torch.long)
    rows = torch.empty_like(logits, dtype=torch.float32)
    logp = torch.zeros(R, dtype=torch.float32)
    fgap, dgap, n_done = [np.inf] * R, [np.inf] * R, 0
    for r in range(R):
        pr = process_row(logits[r], seqs[r, :cur_len].tolist(), eos, opts)
        rows[r], fgap[r] = pr['row'], pr['gap']
        tok, lp, dgap[r] = choose(pr['row'], opts['do_sample'], None if uniforms is None else uniforms[r, cur_len], pad)
        if not unfinished[r]:
            tok, lp = pad, 0.0
        elif tok == eos:
            unfinished[r] = False
            n_done += 1
        words[r], logp[r] = tok, lp
    seqs[:, cur_len] = words
    return dict(words=words, rows=rows, tok_logp=logp, filter_gap=fgap, draw_gap=dgap, n_done=n_done)


def generate(logits_fn, R, max_len, bos, eos, pad, opts, uniforms=None):
    """the whole token loop: logits_fn(t, seqs) -> (R, V) f32 raw logits of the step that chooses column t + 1 (t = 0: every row holds
    [BOS] only) -> dict(seqs (R, max_len) int64 padded with `pad`, tok_logp (R, max_len) f32 (column 0 = 0), lengths (R,) = columns up to
    and including [EOS], min_filter_gap, min_draw_gap over the unfinished rows, steps = steps until every row had finished)"""
    seqs = torch.full((R, max_len), pad, dtype=torch.long)
    seqs[:, 0] = bos
    unfinished = torch.ones(R, dtype=torch.bool)
    tok_logp = torch.zeros(R, max_len, dtype=torch.float32)
    lengths = torch.full((R,), max_len, dtype=torch.long)
    fg, dg, steps = np.inf, np.inf, None
    for t in range(max_len - 1):
        live = unfinished.clone()
        st = step(logits_fn(t, seqs), seqs, unfinished, t + 1, eos, pad, opts, uniforms)
        tok_logp[:, t + 1] = st['tok_logp']
        for r in range(R):
            if live[r]:
                fg, dg = min(fg, st['filter_gap'][r]), min(dg, st['draw_gap'][r])
                if not unfinished[r]:
                    lengths[r] = t + 2
        if steps is None and not unfinished.any():
            steps = t + 1
    return dict(seqs=seqs, tok_logp=tok_logp, lengths=lengths, min_filter_gap=fg, min_draw_gap=dg, steps=steps)


def pack(seqs, lengths):
    """the session's packed result: ids | length in columns"""
    return torch.cat([seqs, lengths.view(-1, 1)], dim=1)
