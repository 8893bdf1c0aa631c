"""Test infrastructure: tests/hf_beam_restatement.py:HFBeam generalised to what Hugging Face's `generate` adds to a beam search on request, in
the state layout of evk_hf_beam_step_opts (csrc/hf_beam.hip), so that a GPU test can compare after every token.

  * The logits processors act in beam mode on the rows AFTER log_softmax, on every running beam's row from that beam's own history
    ([BOS] included), in HF's order: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor -- the row
    arithmetic is tests/hf_sample_restatement.py:process_row (f32, a ban wins over a penalty on the same id).
  * A hypothesis score is float(sum) / D[cur_len] with D[c] = c ** length_penalty (Python floats); the same divisor serves the done test.
  * A study is done when its list is full and (early_stopping or worst >= best / D[cur_len]).
Everything else -- candidates, ranking, ties, rank walk, insertion, eviction, force_end, frozen done studies -- is HFBeam's.

Also here: `sticky_rows`, the synthetic rows of the GPU tests with a few study-dependent ids boosted so that tokens and bigrams recur (on
plain random rows no processor would ever change a decision), and what the trace needs for the CPU preconditions of those tests."""
import math

import torch

from tests.hf_beam_restatement import HFBeam
from tests.hf_sample_restatement import options as sample_options, process_row

NEUTRAL = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_length=0, length_penalty=1.0, early_stopping=False)
PROCESSORS = ('repetition_penalty', 'no_repeat_ngram_size', 'min_length')


def options(**kw):
    bad = set(kw) - set(NEUTRAL)
    assert not bad, bad
    return dict(NEUTRAL, **kw)


def length_divisors(length_penalty, max_len):
    """D[c] = c ** length_penalty for c = 0 .. max_len: what the engine computes on the host and hands to the kernel as f64"""
    lp = float(length_penalty)
    return [(float(c) ** lp) if c or lp >= 0 else float('inf') for c in range(max_len + 1)]          # (D[0] is never read)


def process_rows(logp, seqs, cur_len, nb, done, eos, opts, V):
    """the three processors on the (R, >= V) f32 rows of every study that is not done -> a processed copy (the other rows and the
    columns beyond V as they were)"""
    out = logp.clone()
    so = sample_options(**{k: opts[k] for k in PROCESSORS})
    for r in range(logp.shape[0]):
        if done[r // nb]:
            continue
        out[r, :V] = process_row(logp[r, :V], seqs[r, :cur_len].tolist(), eos, so)['row']
    return out


class HFBeamOpts(HFBeam):
    def __init__(self, B, nb, V, max_len, bos, eos, pad, opts=None, anc_cols=None, done_test='candidate'):
        super().__init__(B, nb, V, max_len, bos, eos, pad, anc_cols=anc_cols, done_test=done_test)
        self.opts = options(**(opts or {}))
        self.div = length_divisors(self.opts['length_penalty'], max_len)
        self.rows = None                            # the processed rows of the last step (what the kernel leaves in logp)

    def _top(self, logp):
        cand = (self.scores.view(-1, 1) + logp[:, :self.V].float()).view(self.B, self.nb * self.V)
        return torch.sort(cand, dim=1, descending=True, stable=True)

    def step(self, logp, force_end=False):
        """HFBeam.step on the processed rows, with the divisor table and early_stopping"""
        B, nb, V, pos = self.B, self.nb, self.V, self.pos
        cur_len, D = pos + 1, self.div[pos + 1]
        live = [b for b in range(B) if not self.done[b]]
        raw = logp[:, :V].float()
        logp = process_rows(raw, self.seqs, cur_len, nb, self.done, self.eos, self.opts, V)
        self.rows = logp
        top_s, top_i = self._top(logp)
        # per switched-on processor: live studies whose 2 * nb best candidates become another set when that processor alone acts on the raw
        # rows of this state (alone: where a ban covers a penalised id, the penalty cannot show in the company of the ban)
        changed, raw_i = {}, self._top(raw)[1]
        for k in PROCESSORS:
            if self.opts[k] != NEUTRAL[k]:
                one_i = self._top(process_rows(raw, self.seqs, cur_len, nb, self.done, self.eos, dict(NEUTRAL, **{k: self.opts[k]}), V))[1]
                changed[k] = sum(int(set(one_i[b, :2 * nb].tolist()) != set(raw_i[b, :2 * nb].tolist())) for b in live)
        finite = min([int(torch.isfinite(top_s[b]).sum()) for b in live] or [nb * V])
        gap = float((top_s[live, :2 * nb] - top_s[live, 1:2 * nb + 1]).min()) if live and nb * V > 2 * nb else float('inf')
        if gap != gap:                              # (-inf next to -inf: no margin to speak of)
            gap = 0.0
        top_s, top_i = top_s[:, :2 * nb], top_i[:, :2 * nb]
        new_seqs, new_anc = self.seqs.clone(), (self.anc.clone() if self.anc is not None else None)
        tr = dict(eos_taken=0, eos_skipped=0, evicted=0, forced=0, later_hf_differs=0, min_gap=gap, changed=changed, finite=finite,
                  live=len(live))
        for b in range(B):
            rows = slice(b * nb, (b + 1) * nb)
            if self.done[b]:
                new_seqs[rows] = self.seqs[b * nb]
                new_seqs[rows, pos + 1] = self.pad
                if new_anc is not None:
                    new_anc[rows] = self.anc[b * nb]
                self.scores[b] = 0.0
                self.words[rows] = self.pad
                continue
            k = 0
            nxt = []
            for rank in range(2 * nb):
                flat, sc = int(top_i[b, rank]), float(top_s[b, rank])
                tok, src = flat % V, flat // V
                if tok == self.eos:
                    if rank >= nb:
                        tr['eos_skipped'] += 1
                        continue
                    toks = self.seqs[b * nb + src, :pos + 1].tolist() + [tok]
                    tr['evicted'] += self._insert(b, (sc / D, pos + 2, toks))
                    tr['eos_taken'] += 1
                else:
                    nxt.append((top_s[b, rank].clone(), tok, src))
                    k += 1
                if k == nb:
                    break
            assert k == nb
            for j, (sc, tok, src) in enumerate(nxt):
                r = b * nb + j
                new_seqs[r] = self.seqs[b * nb + src]
                new_seqs[r, pos + 1] = tok
                if new_anc is not None:
                    new_anc[r] = self.anc[b * nb + src]
                self.scores[b, j] = sc
                self.words[r] = tok
            full = len(self.hyps[b]) >= nb
            early = bool(self.opts['early_stopping'])
            if full and not early and (self.hyps[b][-1][0] >= float(nxt[0][0]) / D) != (self.hyps[b][-1][0] >= float(top_s[b, 0]) / D):
                tr['later_hf_differs'] += 1
            best = top_s[b, 0] if self.done_test == 'candidate' else nxt[0][0]
            if full and (early or self.hyps[b][-1][0] >= float(best) / D):
                self.done[b] = True
            elif force_end:
                for j in range(nb):
                    self._insert(b, (float(self.scores[b, j]) / D, pos + 2, new_seqs[b * nb + j, :pos + 2].tolist()))
                tr['forced'] += 1
        if new_anc is not None and pos + 1 < new_anc.shape[1]:
            new_anc[:, pos + 1] = torch.arange(B * nb, dtype=torch.int32)
        self.seqs, self.anc = new_seqs, new_anc
        self.pos = pos + 1
        tr['done'] = list(self.done)
        self.trace.append(tr)


def hf_beam_search_opts(logp_fn, B, nb, V, max_len, bos, eos, pad, opts, n=1, stop_when_done=True, done_test='candidate'):
    """the whole search: logp_fn(step, seqs) -> (R, V) f32 log-probability rows for the tokens in column `step`
    -> (sequences (B*n, L), scores (B*n,) f64, trace)"""
    st = HFBeamOpts(B, nb, V, max_len, bos, eos, pad, opts, done_test=done_test)
    for t in range(max_len - 1):
        st.step(logp_fn(t, st.seqs), force_end=(t == max_len - 2))
        if stop_when_done and all(st.done):
            break
    seqs, scores = st.result(n)
    return seqs, scores, st.trace


N_STICKY = 3


def default_boost(V):
    """the boost at which a sticky id competes with the largest of the V - 3 other logits (standard deviation 2: their maximum is
    about 2 * sqrt(2 ln V)) instead of drowning among them"""
    return 2.0 * math.sqrt(2.0 * math.log(V))


def sticky_rows(seed, step, R, V, eos, nb, schedule, boost=None, n_sticky=N_STICKY):
    """tests/hf_beam_restatement.py:synthetic_rows with `boost` added, before the log_softmax, to the logits of n_sticky ids that depend on
    the study only (never 0, [BOS] or [EOS]): the same few tokens stay likely at every step of a study, so ids and bigrams recur and the
    processors have something to act on.  A function of (seed, step, flat row) only."""
    if boost is None:
        boost = default_boost(V)
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(step)) * 7919 + 17)
    x = torch.randn(R, V, generator=g, dtype=torch.float32) * 2.0
    for r in range(R):
        b = r // nb
        t0, amt = schedule[b % len(schedule)]
        if step >= t0:
            x[r, eos] += amt
        for i in range(n_sticky):
            x[r, 1 + (7 * b + 11 * i + 3 * int(seed)) % (V - 3)] += boost
    return torch.log_softmax(x, dim=-1)
