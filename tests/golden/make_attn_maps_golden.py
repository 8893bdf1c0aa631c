#!/usr/bin/env python3
"""Fixture of the decoder's cross-attention maps, written by the imported reference on the CPU:

  tests/golden/beam224_b4_attn.npz     the reference FineTune on case beam224_b4 (procedural weights, zero dropout).  `enc` f32 (B, S, 512):
      the encoder states its decoder attends to (Transformer.encode's output: the global token is dropped in front of it, so S = 7 x 7).
      Then, for two sets of ids -- `beam`: the beam result eval/seq of beam224_b4.npz, `greedy`: the ids of sample224_greedy.npz -- a
      teacher-forced Transformer.decode on [BOS] + ids:
        <set>/ids      int64 (B, L)
        <set>/maps     f32 (B, L, n_layers, S): the head mean of decoder.layers[i].src_attn.attn (MultiHeadedAttention.attn,
                       modules/encoder_decoder.py:189,200); row t is the map of the step that scores word t
        <set>/drift16  same shape: |maps - the same run with every 2-D decoder weight and `enc` rounded to fp16|, the rule of
                       make_beam_trace.py::drift16 applied to the maps: an engine with 16-bit operands cannot be closer to the reference
                       than the reference is to itself in 16 bits

Usage (build container only: needs the reference checkout):  python tests/golden/make_attn_maps_golden.py
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.cases import CASES, make_inputs  # noqa: E402
from tests.golden.make_golden import REF, install_shims, load_procedural, make_args, zero_dropout  # noqa: E402
from oracle import spec as S  # noqa: E402

BASE = 'beam224_b4'


def forced_maps(td, enc, ids, bos):
    """teacher-forced decode of [BOS] + ids over the encoder states `enc` -> (B, L, n_layers, S) head-mean cross-attention maps"""
    from modules.encoder_decoder import subsequent_mask
    tgt = torch.cat([torch.full((ids.shape[0], 1), bos, dtype=torch.long), ids[:, :-1]], 1)
    src_mask = torch.ones(enc.shape[0], 1, enc.shape[1], dtype=torch.long)
    tgt_mask = torch.ones_like(tgt).unsqueeze(-2) & subsequent_mask(tgt.size(-1)).to(tgt)
    td.model.decode(enc, src_mask, tgt, tgt_mask)
    return torch.stack([l.src_attn.attn.mean(1) for l in td.model.decoder.layers], 2)


def main():
    from modules.tokenizers_new import build_my_tokenizer
    from models.model_pretrain_finetune_v0623_large_res import FineTune
    tokenizer = build_my_tokenizer(os.path.join(REF, 'config/tokenizer'), data_name='iu_xray')
    V = tokenizer.get_vocab_size()
    tmp = os.path.join(tempfile.gettempdir(), 'evoke_golden')
    os.makedirs(tmp, exist_ok=True)
    case = CASES[BASE]
    inp = make_inputs(case, V)
    args = make_args(tmp, tokenizer, case['max_seq_len'], case['beam_size'], case.get('multiview', True))
    model = FineTune(args, tokenizer, 'iu_xray')
    load_procedural(model, S.finetune_spec(V))
    zero_dropout(model)
    model.eval()
    td = model.text_decoder
    got = {}
    h = td.model.encoder.register_forward_hook(lambda m, i, o: got.update(enc=o.detach().clone()))
    with torch.no_grad():
        _, seq = model(inp['images'], inp['ids'], inp['masks'], np.array(inp['patient_ids']), inp.get('inc_ids'), inp.get('inc_masks'),
                       mode='inference')
    h.remove()
    gold = np.load(os.path.join(HERE, BASE + '.npz'))
    assert seq.tolist() == gold['eval/seq'].tolist(), 'the reference no longer returns the ids of %s.npz' % BASE
    enc = got['enc'].float()
    half = lambda t: t.half().float()          # noqa: E731
    td16 = copy.deepcopy(td)
    with torch.no_grad():
        for k, p in td16.named_parameters():
            if p.dim() == 2 and 'lut' not in k:
                p.copy_(half(p))
    out = {'enc': enc.numpy().astype(np.float32)}
    sets = {'beam': torch.from_numpy(gold['eval/seq']), 'greedy': torch.from_numpy(np.load(os.path.join(HERE, 'sample224_greedy.npz'))['seq'])}
    for name, ids in sets.items():
        with torch.no_grad():
            maps = forced_maps(td, enc, ids, V - 2)
            low = forced_maps(td16, half(enc), ids, V - 2)
        out[name + '/ids'] = ids.numpy().astype(np.int64)
        out[name + '/maps'] = maps.numpy().astype(np.float32)
        out[name + '/drift16'] = (low - maps).abs().numpy().astype(np.float32)
        print(name, 'maps', tuple(maps.shape), 'row sums in [%.7f, %.7f]' % (maps.sum(-1).min().item(), maps.sum(-1).max().item()),
              'max drift16 per layer', out[name + '/drift16'].max(axis=(0, 1, 3)), 'largest weight per layer', out[name + '/maps'].max(axis=(0, 1, 3)))
    path = os.path.join(HERE, BASE + '_attn.npz')
    np.savez_compressed(path, **out)
    print('written', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    main()
