#!/usr/bin/env python3
"""Fixtures of the sampling decode route (AttModel._sample, modules/att_model.py:139-224), written by the imported reference on the
CPU with the procedural weights: tests/golden/sample_<case>.npz.  Per case the returned ids `seq` (R, T) and, per row and position, a
digest of the stored log-probability row seqLogprobs[r, t] (the values AFTER the decoding constraint and the trigram penalty): its eight
largest entries (`top_ids`, `top_logp`, descending, ties to the lower index), the entries at PROBE_IDS (`probe_logp`) and the margin
top-1 minus top-2 (`margin`) -- what a 16-bit engine needs to price a disagreement by the reference's own decision margin.

Usage (build container only: needs the reference checkout):  python tests/golden/make_sample_golden.py [case ...]
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import CASES, PROBE_IDS, make_inputs  # noqa: E402
from tests.golden.make_golden import REF, install_shims, load_procedural, make_args, zero_dropout  # noqa: E402
from oracle import spec as S  # noqa: E402

N_TOP = 8

# name -> (case of cases.py that supplies the inputs, the options of AttModel._sample that differ from the shipped configuration)
SAMPLE_CASES = {
    'sample224_greedy': ('beam224', dict(max_seq_len=40, sample_method='greedy', block_trigrams=1)),
    'sample224_n2': ('beam224', dict(max_seq_len=24, sample_method='greedy', block_trigrams=1, sample_n=2)),
    'sample224_constraint': ('beam224', dict(max_seq_len=24, sample_method='greedy', block_trigrams=0, decoding_constraint=1)),
    'sample384_L100': ('beam384_b4_L100', dict(max_seq_len=100, sample_method='greedy', block_trigrams=1)),
}


def digest(seq, logp):
    """seq (R, T) int64, logp (R, T, V+1) -> the arrays of one fixture"""
    lp = logp.detach().float()
    # descending, ties to the lower index: a stable sort of the negated row
    order = torch.sort(-lp, dim=-1, stable=True).indices[..., :N_TOP]
    top = lp.gather(-1, order)
    return {'seq': seq.numpy().astype(np.int64), 'top_ids': order.numpy().astype(np.int32), 'top_logp': top.numpy().astype(np.float32),
            'probe_logp': lp[..., PROBE_IDS].numpy().astype(np.float32), 'margin': (top[..., 0] - top[..., 1]).numpy().astype(np.float32)}


def run_case(name, tmp, tokenizer):
    base, opts = SAMPLE_CASES[name]
    case = CASES[base]
    inp = make_inputs(case, tokenizer.get_vocab_size())
    args = make_args(tmp, tokenizer, opts['max_seq_len'], 1, case.get('multiview', True))
    args.update(dict(sample_n=1, group_size=1, temperature=1.0, decoding_constraint=0, output_logsoftmax=1))
    args.update(opts)
    from models.model_pretrain_finetune_v0623_large_res import FineTune
    model = FineTune(args, tokenizer, 'iu_xray')
    load_procedural(model, S.finetune_spec(tokenizer.get_vocab_size()))
    zero_dropout(model)
    model.eval()
    got = {}
    h = model.text_decoder.register_forward_hook(lambda m, i, o: got.update(out=o))
    with torch.no_grad():
        texts, seq = model(inp['images'], inp['ids'], inp['masks'], np.array(inp['patient_ids']), inp.get('inc_ids'), inp.get('inc_masks'),
                           mode='inference')
    h.remove()
    seq2, logp = got['out']
    assert torch.equal(seq, seq2)
    out = digest(seq, logp)
    out['texts'] = np.array(texts)
    return out


def main(names):
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from modules.tokenizers_new import build_my_tokenizer
    tokenizer = build_my_tokenizer(os.path.join(REF, 'config/tokenizer'), data_name='iu_xray')
    tmp = os.path.join(tempfile.gettempdir(), 'evoke_golden')
    os.makedirs(tmp, exist_ok=True)
    for name in names:
        out = run_case(name, tmp, tokenizer)
        path = os.path.join(HERE, name + '.npz')
        if os.path.exists(path):
            old = np.load(path)
            same = all(np.array_equal(old[k], out[k]) for k in out)
            print(name, 'reproduces the committed fixture' if same else 'DIFFERS from the committed fixture')
        np.savez_compressed(path, **out)
        eos = tokenizer.get_vocab_size() - 1
        print(name, out['seq'].shape, 'positions with margin < 1.6e-2 per row:', (out['margin'] < 1.6e-2).sum(1).tolist(),
              '[EOS] emitted:', bool((out['seq'] == eos).any()))


if __name__ == '__main__':
    main(sys.argv[1:] or list(SAMPLE_CASES))
