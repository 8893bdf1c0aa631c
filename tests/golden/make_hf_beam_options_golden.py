"""Records tests/golden/hf_beam_options_tiny.npz: what the installed Hugging Face `generate` returns for beam searches WITH logits processors
and scorer controls over the tiny GPT-2 cross-attention decoders of make_hf_beam_golden.py, for tests/test_hf_beam_options_cpu.py to hold
the generalised restatement (tests/hf_beam_options_restatement.py) against.  Needs `transformers` only.

    python tests/golden/make_hf_beam_options_golden.py

Cases: weight seed {0, 1} x [EOS] logit offset {0, 3} x num_beams {2, 3, 4, 8} x the eight option sets of OPTION_SETS, with
num_return_sequences = num_beams and max_length 12: 128 cases.  Stored per case: sequences and sequences_scores only -- weights and encoder
outputs are those of hf_beam_tiny.npz (the script asserts that the models it rebuilds equal them), so this fixture stays small.
A case in which the restatement takes some decision by a margin below 1e-5 is not recorded; the script prints what it drops."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

MAX_LENGTH = 12
MARGIN = 1e-5
# (repetition_penalty, no_repeat_ngram_size, min_length, length_penalty, early_stopping)
OPTION_SETS = ((1.3, 0, 0, 1.0, False), (1.0, 2, 0, 1.0, False), (1.0, 0, 5, 1.0, False), (1.2, 3, 4, 1.0, False),
               (1.0, 0, 0, 0.0, False), (1.0, 0, 0, 2.0, False), (1.0, 0, 0, 1.0, True), (1.2, 2, 4, 0.5, True))
KEYS = ('repetition_penalty', 'no_repeat_ngram_size', 'min_length', 'length_penalty', 'early_stopping')


def main():
    from oracle import gpt2 as G
    from tests.golden.make_hf_beam_golden import B, BOS, EOS, HEADS, LAYERS, PAD, V, build
    from tests.hf_beam_options_restatement import hf_beam_search_opts
    base = np.load(os.path.join(HERE, 'hf_beam_tiny.npz'))
    out = dict(option_sets=np.array(OPTION_SETS, dtype=np.float64), max_length=np.array(MAX_LENGTH))
    cases, dropped = [], []
    for seed in (0, 1):
        m = build(seed)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith('transformer.') and not k.endswith(('.attn.bias', '.masked_bias'))}
        for k, v in sd.items():
            assert np.array_equal(base['w%d/%s' % (seed, k)], v.numpy().astype(np.float32)), k          # the models of hf_beam_tiny.npz
        enc = torch.from_numpy(base['enc%d' % seed])
        P = {G.PRE + k: v for k, v in sd.items()}
        offset = [0.0]

        def hook(mod, args, res):
            res.logits[..., EOS] += offset[0]
            return res
        m.register_forward_hook(hook)
        for off in (0.0, 3.0):
            offset[0] = off
            for nb in (2, 3, 4, 8):
                for k, o in enumerate(OPTION_SETS, 1):
                    opts = dict(zip(KEYS, o))
                    with torch.no_grad():
                        r = m.generate(input_ids=torch.full((B, 1), BOS), encoder_hidden_states=enc, num_beams=nb, num_return_sequences=nb,
                                       max_length=MAX_LENGTH, use_cache=True, do_sample=False, output_scores=True, return_dict_in_generate=True,
                                       bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD, repetition_penalty=float(o[0]),
                                       no_repeat_ngram_size=int(o[1]), min_length=int(o[2]), length_penalty=float(o[3]), early_stopping=bool(o[4]))

                    def logp_fn(step, rows, P=P, enc=enc, nb=nb, off=off):
                        h, _ = G.gpt2_hidden(P, rows[:, :step + 1], None, enc.repeat_interleave(nb, 0), HEADS, LAYERS)
                        lg = h[:, -1] @ P[G.PRE + 'transformer.wte.weight'].t()
                        lg[:, EOS] += off
                        return torch.log_softmax(lg, -1)
                    # the decision margins of the restatement over the oracle's log-probabilities, under either done test
                    gap = min(t['min_gap'] for dt in ('running', 'candidate')
                              for t in hf_beam_search_opts(logp_fn, B, nb, V, MAX_LENGTH, BOS, EOS, PAD, opts, n=nb, done_test=dt)[2])
                    name = 's%d_o%d_nb%d_k%d' % (seed, int(off), nb, k)
                    if gap < MARGIN:
                        dropped.append((name, gap))
                        continue
                    cases.append(name)
                    out['case/%s/seq' % name] = r.sequences.numpy().astype(np.int8)
                    out['case/%s/score' % name] = r.sequences_scores.double().numpy()
    out['cases'] = np.array(cases)
    path = os.path.join(HERE, 'hf_beam_options_tiny.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, %d dropped %s, %d bytes' % (path, len(cases), len(dropped), dropped, os.path.getsize(path)))


if __name__ == '__main__':
    main()
