"""Records tests/golden/hf_sample_tiny.npz: what the installed Hugging Face `generate` returns when it samples, or decodes greedily, with its
standard logits processors over the tiny GPT-2 cross-attention decoders of make_hf_beam_golden.py (same build(seed), weights and encoder
inputs: both are read from hf_beam_tiny.npz, not stored again), for tests/test_hf_sample_cpu.py to hold the restatement
(tests/hf_sample_restatement.py) against.  It needs `transformers` only, no reference checkout.

    python tests/golden/make_hf_sample_golden.py

Cases: do_sample with {plain, T 0.7 + top_k 5, T 1.3 + top_p 0.8 + no_repeat_ngram_size 2 + min_length 4, repetition_penalty 1.2 +
no_repeat_ngram_size 3 + top_k 10 + top_p 0.9, top_k 1} x num_return_sequences in {1, 3}, and greedy with {repetition_penalty 1.3,
no_repeat_ngram_size 2, min_length 6, all three}; each x max_length in {6, 12} x an [EOS] logit offset of 0 or 3.0 (a forward hook adds it,
so that rows finish early), on the weights of seed 0.  Stored per case: `seq` = sequences, `scores` = the PROCESSED rows of every step and `logits`
= the raw rows (generate(..., output_scores=True, output_logits=True)) under a fixed torch.manual_seed, and `keep`: a row of a step is left
out of the comparison when the restatement, teacher-forced on the recorded ids and fed the recorded raw logits, takes a filter decision
(top-k boundary, nucleus boundary, greedy arg-max) by a margin below 1e-5 -- such a row tests rounding, not the algorithm.  The script
prints what it drops and refuses to drop more than 5 % of all rows."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

MARGIN = 1e-5
SAMPLED = dict(plain=dict(),
               t07_k5=dict(temperature=0.7, top_k=5),
               t13_p08_g2_min4=dict(temperature=1.3, top_p=0.8, no_repeat_ngram_size=2, min_length=4),
               rp12_g3_k10_p09=dict(repetition_penalty=1.2, no_repeat_ngram_size=3, top_k=10, top_p=0.9),
               k1=dict(top_k=1))
GREEDY = dict(rp13=dict(repetition_penalty=1.3),
              g2=dict(no_repeat_ngram_size=2),
              min6=dict(min_length=6),
              rp13_g2_min6=dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=6))


def main():
    from tests.golden.make_hf_beam_golden import B, BOS, EOS, PAD, V, build
    from tests import hf_sample_restatement as HS
    beam = np.load(os.path.join(HERE, 'hf_beam_tiny.npz'))
    out, cases, options, dropped, n_rows = {}, [], {}, [], 0
    for seed in (0,):
        m = build(seed)
        sd = m.state_dict()
        with torch.no_grad():
            for k in beam.files:
                if k.startswith('w%d/' % seed):
                    sd[k[3:]].copy_(torch.from_numpy(beam[k]))
        m.tie_weights()
        enc = torch.from_numpy(beam['enc%d' % seed])
        offset = [0.0]

        def hook(mod, args, res):
            res.logits[..., EOS] += offset[0]
            return res
        m.register_forward_hook(hook)
        grid = [(True, name, o, n) for name, o in SAMPLED.items() for n in (1, 3)] + [(False, name, o, 1) for name, o in GREEDY.items()]
        for off in (0.0, 3.0):
            offset[0] = off
            for do_sample, oname, o, n in grid:
                for ml in (6, 12):
                    opts = HS.options(do_sample=do_sample, **o)
                    name = 's%d_o%d_%s_%s_n%d_ml%d' % (seed, int(off), 'sample' if do_sample else 'greedy', oname, n, ml)
                    torch.manual_seed(1000 + len(cases))
                    with torch.no_grad():
                        r = m.generate(input_ids=torch.full((B, 1), BOS), encoder_hidden_states=enc, num_beams=1, num_return_sequences=n,
                                       max_length=ml, use_cache=True, do_sample=do_sample, temperature=opts['temperature'], top_k=opts['top_k'],
                                       top_p=opts['top_p'], repetition_penalty=opts['repetition_penalty'],
                                       no_repeat_ngram_size=opts['no_repeat_ngram_size'], min_length=opts['min_length'], output_scores=True,
                                       output_logits=True, return_dict_in_generate=True, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=PAD)
                    seq = r.sequences
                    scores, logits = torch.stack(r.scores).float(), torch.stack(r.logits).float()          # (steps, B * n, V)
                    keep = np.ones(scores.shape[:2], dtype=bool)
                    for t in range(scores.shape[0]):
                        for row in range(seq.shape[0]):
                            gap = HS.process_row(logits[t, row], seq[row, :t + 1].tolist(), EOS, opts)['gap']
                            if gap < MARGIN:
                                keep[t, row] = False
                                dropped.append((name, t, row, gap))
                    n_rows += keep.size
                    cases.append(name)
                    options[name] = dict(opts, n=n, max_length=ml, eos_offset=off, seed=seed)
                    out['case/%s/seq' % name] = seq.numpy().astype(np.int64)
                    out['case/%s/scores' % name] = scores.numpy().astype(np.float32)
                    out['case/%s/logits' % name] = logits.numpy().astype(np.float32)
                    out['case/%s/keep' % name] = keep
    assert len(dropped) <= 0.05 * n_rows, (len(dropped), n_rows)
    out['cases'] = np.array(cases)
    out['options'] = np.array(json.dumps(options))
    out['dims'] = np.array([V, B, BOS, EOS, PAD], dtype=np.int64)
    path = os.path.join(HERE, 'hf_sample_tiny.npz')
    np.savez_compressed(path, **out)
    print('%s: %d cases, %d rows, %d dropped %s, %d bytes' % (path, len(cases), n_rows, len(dropped), dropped, os.path.getsize(path)))


if __name__ == '__main__':
    main()
