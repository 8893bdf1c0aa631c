"""Records tests/golden/hf_beam_tiny.npz: what the installed Hugging Face `generate` returns for beam searches over tiny GPT-2
cross-attention decoders (two layers, width 32, 4 heads, vocabulary 40, B = 3 studies, S = 5 encoder positions), for
tests/test_hf_beam_cpu.py to hold the classic-algorithm restatement (tests/hf_beam_restatement.py) against.  Separate from make_golden.py:
it needs `transformers` only, no reference checkout.

    python tests/golden/make_hf_beam_golden.py

Cases: num_beams in {1, 2, 3, 4, 8} x num_return_sequences in {1, num_beams} x max_length in {6, 12} x an [EOS] logit offset of 0 or 3.0
(a forward hook on the model adds it, so that hypotheses finish early) x two weight seeds.  Stored per case: sequences and
sequences_scores.  num_beams 1 is greedy search, for which `generate` reports no sequences_scores: the score stored is the one the beam
scorer would give that sequence, sum of the chosen tokens' log-probabilities (from the recorded per-step scores) / generated length.
A case in which the restatement driven by oracle.gpt2 takes some decision by a margin below 1e-5 is not recorded (HF and the oracle
differ by ~1e-6 in the log-probabilities; such a case tests rounding, not the algorithm): the script prints what it drops.

`later_hf_differs` names the cases in which, somewhere along the search, the done test of the classic BeamSearchScorer (the reference pins
transformers 4.23.1: worst kept hypothesis >= BEST CANDIDATE / length, the candidate possibly an [EOS]) and the one of the vectorised beam
search of later releases (>= best RUNNING beam / length; the release installed when this was recorded, 5.15, has it) give different
answers.  From that step on the two releases keep different hypothesis lists, so the tails of an n-best result may differ between them.
The list is recorded for information: the test holds every case in full with the restatement's done test switched to the later
release's, and derives the cases in which the two never disagree from the restatement's own trace."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

V, D, LAYERS, HEADS, B, S = 40, 32, 2, 4, 3, 5
BOS, EOS, PAD = V - 2, V - 1, 0
MARGIN = 1e-5


def build(seed):
    from transformers import GPT2Config, GPT2LMHeadModel
    torch.manual_seed(seed)
    cfg = GPT2Config(vocab_size=V, n_embd=D, n_layer=LAYERS, n_head=HEADS, n_positions=32, add_cross_attention=True, is_decoder=True,
                     bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, initializer_range=0.35)
    m = GPT2LMHeadModel(cfg)
    with torch.no_grad():
        # (whatever the installed version initialises: every weight is drawn here, biases and norms included)
        for name, p in m.named_parameters():
            p.copy_(torch.randn(p.shape) * (0.35 if p.dim() > 1 else 0.1))
            if '.ln_' in name and name.endswith('weight'):
                p.add_(1.0)
    m.tie_weights()
    return m.eval()


def main():
    from oracle import gpt2 as G
    from tests.hf_beam_restatement import hf_beam_search
    out = dict(dims=np.array([V, D, LAYERS, HEADS, B, S, BOS, EOS, PAD], dtype=np.int64))
    cases, dropped, differs = [], [], []
    for seed in (0, 1):
        m = build(seed)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith('transformer.') and not k.endswith(('.attn.bias', '.masked_bias'))}
        for k, v in sd.items():
            out['w%d/%s' % (seed, k)] = v.numpy().astype(np.float32)
        enc = torch.randn(B, S, D, generator=torch.Generator().manual_seed(100 + seed))
        out['enc%d' % seed] = enc.numpy().astype(np.float32)
        P = {G.PRE + k: v for k, v in sd.items()}
        offset = [0.0]

        def hook(mod, args, res):
            res.logits[..., EOS] += offset[0]
            return res
        m.register_forward_hook(hook)
        for off in (0.0, 3.0):
            offset[0] = off
            for nb in (1, 2, 3, 4, 8):
                for n in sorted({1, nb}):
                    for ml in (6, 12):
                        with torch.no_grad():
                            r = m.generate(input_ids=torch.full((B, 1), BOS), encoder_hidden_states=enc, num_beams=nb, num_return_sequences=n,
                                           max_length=ml, use_cache=True, do_sample=False, output_scores=True, return_dict_in_generate=True,
                                           bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, length_penalty=1.0, early_stopping=False)
                        seqs = r.sequences
                        if nb == 1:
                            sc = torch.zeros(B, dtype=torch.float64)
                            for b in range(B):
                                tot, ln = 0.0, 0
                                for t, step in enumerate(r.scores):
                                    tok = int(seqs[b, t + 1])
                                    tot += float(torch.log_softmax(step[b].float(), -1)[tok])
                                    ln += 1
                                    if tok == EOS:
                                        break
                                sc[b] = tot / ln
                        else:
                            sc = r.sequences_scores.double()

                        # the decision margins of the restatement over the oracle's log-probabilities
                        def logp_fn(step, rows, P=P, enc=enc, nb=nb, off=off):
                            h, _ = G.gpt2_hidden(P, rows[:, :step + 1], None, enc.repeat_interleave(nb, 0), HEADS, LAYERS)
                            lg = h[:, -1] @ P[G.PRE + 'transformer.wte.weight'].t()
                            lg[:, EOS] += off
                            return torch.log_softmax(lg, -1)
                        _, _, trace = hf_beam_search(logp_fn, B, nb, V, ml, BOS, EOS, PAD, n=n)
                        gap = min(t['min_gap'] for t in trace)
                        name = 's%d_o%d_nb%d_n%d_ml%d' % (seed, int(off), nb, n, ml)
                        if gap < MARGIN:
                            dropped.append((name, gap))
                            continue
                        cases.append(name)
                        if sum(t['later_hf_differs'] for t in trace):
                            differs.append(name)
                        out['case/%s/seq' % name] = seqs.numpy().astype(np.int64)
                        out['case/%s/score' % name] = sc.numpy().astype(np.float64)
    out['cases'] = np.array(cases)
    out['later_hf_differs'] = np.array(differs)
    path = os.path.join(HERE, 'hf_beam_tiny.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases (%d with a done test that depends on the release), %d dropped %s, %d bytes'
          % (path, len(cases), len(differs), len(dropped), dropped, os.path.getsize(path)))


if __name__ == '__main__':
    main()
