"""Test infrastructure: the classic Hugging Face BeamSearchScorer (length_penalty 1, early_stopping False) restated step by step, in the
state layout of evk_hf_beam_step (csrc/hf_beam.hip), so that a GPU test can compare after every token.  The algorithm is the host loop of
evoke_amd/gpt2.py:_generate_host, i.e. oracle/gpt2.py:beam_search, extended by what that loop throws away: the whole sorted hypothesis list
of every study (num_return_sequences) and its scores (sequences_scores).

Arithmetic as the reference's: candidate = running sum + log-probability in f32, 2 * nb largest in descending order (ties: lowest flat
index), hypothesis score = float(sum) / cur_len in Python floats (f64), list kept by a stable sort on the score, cut to nb.

Also here: the synthetic log-probability rows the GPU tests feed through the step hook (a function of seed, step and flat row only)."""
import torch


class HFBeam:
    def __init__(self, B, nb, V, max_len, bos, eos, pad, anc_cols=None, done_test='candidate'):
        # done_test: what the list's worst entry is compared with -- 'candidate', the best candidate of the step, possibly an [EOS] (the classic
        # scorer of the reference's pinned transformers 4.23.1, what evk_hf_beam_step follows), or 'running', the best running beam after the
        # step (the vectorised beam search of later releases).  Nothing else differs between the two.
        assert done_test in ('candidate', 'running')
        self.done_test = done_test
        self.B, self.nb, self.V, self.max_len, self.bos, self.eos, self.pad = B, nb, V, max_len, bos, eos, pad
        R = B * nb
        self.seqs = torch.full((R, max_len), pad, dtype=torch.long)
        self.seqs[:, 0] = bos
        self.scores = torch.zeros(B, nb, dtype=torch.float32)
        self.scores[:, 1:] = -1e9
        self.words = torch.full((R,), bos, dtype=torch.long)
        self.anc = None
        if anc_cols is not None:
            self.anc = torch.arange(R, dtype=torch.int32).view(R, 1).expand(R, anc_cols).contiguous()
        self.hyps = [[] for _ in range(B)]          # per study: (score, columns, [tokens]) sorted by score descending, at most nb
        self.done = [False] * B
        self.pos = 0                                # last filled column of seqs
        self.trace = []                             # per step: dict(done, eos_taken, eos_skipped, evicted, forced, later_hf_differs, min_gap)

    def _insert(self, b, entry):
        """-> 1 when a full list lost an entry to this one"""
        full = len(self.hyps[b]) >= self.nb
        merged = sorted(self.hyps[b] + [entry], key=lambda x: -x[0])          # stable: an equal score stays behind the earlier entry
        self.hyps[b] = merged[:self.nb]
        return int(full and any(e is entry for e in self.hyps[b]))

    def step(self, logp, force_end=False):
        """logp (R, >= V) f32: the rows of the tokens in column self.pos"""
        B, nb, V, pos = self.B, self.nb, self.V, self.pos
        cur_len = pos + 1
        cand = (self.scores.view(-1, 1) + logp[:, :V].float()).view(B, nb * V)              # f32 add
        top_s, top_i = torch.sort(cand, dim=1, descending=True, stable=True)
        live = [b for b in range(B) if not self.done[b]]          # (the rows of a done study are copies of one row: ties that decide nothing)
        gap = float((top_s[live, :2 * nb] - top_s[live, 1:2 * nb + 1]).min()) if live and nb * V > 2 * nb else float('inf')
        top_s, top_i = top_s[:, :2 * nb], top_i[:, :2 * nb]
        new_seqs, new_anc = self.seqs.clone(), (self.anc.clone() if self.anc is not None else None)
        tr = dict(eos_taken=0, eos_skipped=0, evicted=0, forced=0, later_hf_differs=0, min_gap=gap)
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
                    tr['evicted'] += self._insert(b, (sc / cur_len, pos + 2, toks))
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
            # transformers releases after the reference's pinned 4.23.1 compare the list's worst entry with the best RUNNING beam instead
            # of the best candidate (which may be an [EOS]): where the two tests disagree the releases' n-best tails may differ
            if len(self.hyps[b]) >= nb and (self.hyps[b][-1][0] >= float(nxt[0][0]) / cur_len) != (self.hyps[b][-1][0] >= float(top_s[b, 0]) / cur_len):
                tr['later_hf_differs'] += 1
            best = top_s[b, 0] if self.done_test == 'candidate' else nxt[0][0]
            if len(self.hyps[b]) >= nb and self.hyps[b][-1][0] >= float(best) / cur_len:
                self.done[b] = True
            elif force_end:
                for j in range(nb):
                    self._insert(b, (float(self.scores[b, j]) / cur_len, pos + 2, new_seqs[b * nb + j, :pos + 2].tolist()))
                tr['forced'] += 1
        if new_anc is not None and pos + 1 < new_anc.shape[1]:
            new_anc[:, pos + 1] = torch.arange(B * nb, dtype=torch.int32)
        self.seqs, self.anc = new_seqs, new_anc
        self.pos = pos + 1
        tr['done'] = list(self.done)
        self.trace.append(tr)

    def lists(self):
        """-> hyp_score (B, nb) f64 (empty slots: nan), hyp_len (B, nb) int32, hyp_seq (B, nb, max_len) int64 padded"""
        B, nb = self.B, self.nb
        score = torch.full((B, nb), float('nan'), dtype=torch.float64)
        ln = torch.zeros(B, nb, dtype=torch.int32)
        seq = torch.full((B, nb, self.max_len), self.pad, dtype=torch.long)
        for b in range(B):
            for k, (s, n_, toks) in enumerate(self.hyps[b]):
                score[b, k], ln[b, k] = s, n_
                seq[b, k, :n_] = torch.tensor(toks)
        return score, ln, seq

    def result(self, n=1):
        """what generate(num_return_sequences=n, return_scores=True) returns: ((B*n, L) ids, (B*n,) f64 scores)"""
        score, ln, seq = self.lists()
        L = min(int(ln[:, :n].max()), self.max_len)
        return seq[:, :n, :L].reshape(self.B * n, L).clone(), score[:, :n].reshape(-1).clone()


def hf_beam_search(logp_fn, B, nb, V, max_len, bos, eos, pad, n=1, stop_when_done=True, done_test='candidate'):
    """the whole search: logp_fn(step, seqs) -> (R, V) f32 rows for the tokens in column `step` of seqs (R, max_len)
    -> (sequences (B*n, L), scores (B*n,) f64, trace)"""
    st = HFBeam(B, nb, V, max_len, bos, eos, pad, done_test=done_test)
    for t in range(max_len - 1):
        st.step(logp_fn(t, st.seqs), force_end=(t == max_len - 2))
        if stop_when_done and all(st.done):
            break
    seqs, scores = st.result(n)
    return seqs, scores, st.trace


def synthetic_rows(seed, step, R, V, eos, nb, schedule):
    """(R, V) f32 log-probabilities of `step`: log_softmax of a hash of (seed, step, row, column), the [EOS] logit of study b's rows raised
    by schedule[b][1] from step schedule[b][0] on.  A function of (seed, step, flat row) only -- it does not look at the hypotheses."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(step)) * 7919 + 17)
    x = torch.randn(R, V, generator=g, dtype=torch.float32) * 2.0
    for r in range(R):
        t0, amt = schedule[(r // nb) % len(schedule)]
        if step >= t0:
            x[r, eos] += amt
    return torch.log_softmax(x, dim=-1)


# (first step, [EOS] logit offset) per study of the GPU tests: study 0 ends early, study 1 never sees a likely [EOS] and is closed by
# force_end, study 2 has a moderately likely [EOS]: candidates beyond rank nb, and late hypotheses that evict earlier ones
SCHEDULE = ((1, 7.0), (0, -30.0), (1, 3.0))
