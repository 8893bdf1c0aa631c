#!/usr/bin/env python3
"""Fixtures of beam search with the reference's working option set (group_size 1: temperature, decoding_constraint, length_penalty,
sample_n = beam_size), written by the imported reference on the CPU:

  tests/golden/beam_options_stub.npz   CaptionModel.beam_search itself (modules/caption_model.py:26-202), driven by a table-driven stub
      `get_logprobs_state` whose log-probabilities are a fixed function of position and last word, with [EOS] made likelier with position
      -- an untrained network never emits [EOS], so only a stub lets the finished list, the length penalty and the ranking show.  Per
      geometry the table and the start words; per geometry and option set the finished lists: ids, scores (f64), lengths, and the stored
      `logps` at the chosen word and at the previous word (the constraint's -inf column).
  tests/golden/beam224_b4_opts.npz     the reference FineTune on case beam224_b4 under four option sets: ids, list scores, lengths and
      seqLogprobs reduced to the chosen-word column and the PROBE_IDS columns.

Usage (build container only: needs the reference checkout):  python tests/golden/make_golden_beam_options.py [stub] [model]
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

# geometry name -> B, beam, max_len, V1 (not a multiple of 8), [EOS] id
STUB_GEOMS = {
    'g3x3_L24': dict(B=3, beam=3, max_len=24, V1=23, eos=21),
    'g2x4_L16': dict(B=2, beam=4, max_len=16, V1=37, eos=35),
    'g1x4_L2': dict(B=1, beam=4, max_len=2, V1=11, eos=9),
}
STUB_OPTS = {
    'default': {},
    'avg_0': dict(length_penalty='avg_0'),
    'wu_0.9': dict(length_penalty='wu_0.9'),
    'temp_0.5': dict(temperature=0.5),
    'temp_2': dict(temperature=2.0),
    'constraint': dict(decoding_constraint=1),
    'all': dict(length_penalty='wu_0.9', temperature=2.0, decoding_constraint=1),
}
MODEL_BASE = 'beam224_b4'
MODEL_OPTS = {
    'nbest': dict(sample_n=4),
    'temp_3': dict(temperature=3.0),
    'constraint': dict(decoding_constraint=1),
    'all_wu': dict(sample_n=4, temperature=3.0, decoding_constraint=1, length_penalty='wu_0.9'),
}


def stub_table(g, seed):
    """(max_len, V1, V1) f32 log-probabilities: row [t][last word]; the [EOS] logit grows with the position"""
    rs = np.random.RandomState(seed)
    logits = rs.standard_normal((g['max_len'], g['V1'], g['V1'])).astype(np.float32) * 1.5
    t = np.arange(g['max_len'], dtype=np.float32)
    logits[:, :, g['eos']] += (0.45 * t - 2.5)[:, None]
    return torch.log_softmax(torch.from_numpy(logits), -1).numpy()


def run_stub(g, table, start, opts):
    from modules.caption_model import CaptionModel

    class Stub(CaptionModel):
        def __init__(self):
            super().__init__()
            self.vocab_size, self.max_seq_length, self.eos_idx = g['V1'] - 1, g['max_len'], g['eos']
            self.table = torch.from_numpy(table)

        def get_logprobs_state(self, it, dummy, state):
            t = min(int(state[0][0, 0, 0]) + 1, g['max_len'] - 1)          # (the reference asks once more after the last position)
            return self.table[t][it].clone(), [state[0] + 1]

    m = Stub()
    B, beam = g['B'], g['beam']
    opt = dict(beam_size=beam, group_size=1, temperature=1.0, decoding_constraint=0, length_penalty='', suppress_UNK=0)
    opt.update(opts)
    init = torch.from_numpy(table)[0][torch.as_tensor(start)].clone()
    done = m.beam_search([torch.zeros(1, B, 1)], init, torch.zeros(B * beam, 1), opt=opt)
    T = g['max_len']
    ids = np.zeros((B, beam, T), dtype=np.int64)
    scores = np.zeros((B, beam), dtype=np.float64)
    lens = np.zeros((B, beam), dtype=np.int32)
    chosen = np.zeros((B, beam, T), dtype=np.float32)
    prev = np.zeros((B, beam, T), dtype=np.float32)
    for b in range(B):
        assert len(done[b]) == beam
        for k, e in enumerate(done[b]):
            n = e['seq'].shape[0]
            ids[b, k, :n], scores[b, k], lens[b, k] = e['seq'].numpy(), e['p'], n
            chosen[b, k, :n] = e['logps'].gather(1, e['seq'].unsqueeze(1))[:, 0].numpy()
            if n > 1:
                prev[b, k, 1:n] = e['logps'][1:].gather(1, e['seq'][:-1].unsqueeze(1))[:, 0].numpy()
    return dict(ids=ids, scores=scores, lens=lens, chosen=chosen, prev=prev)


def make_stub():
    out = {}
    for gi, (gname, g) in enumerate(STUB_GEOMS.items()):
        table = stub_table(g, 100 + gi)
        start = np.array([(3 + 5 * b) % (g['V1'] - 2) for b in range(g['B'])], dtype=np.int64)
        out[gname + '/table'], out[gname + '/start'] = table, start
        base = None
        for oname, opts in STUB_OPTS.items():
            r = run_stub(g, table, start, opts)
            for k, v in r.items():
                out['%s/%s/%s' % (gname, oname, k)] = v
            base = r if base is None else base
            print(gname, oname, 'lengths', r['lens'].tolist(), 'same ids as default:', bool(np.array_equal(r['ids'], base['ids'])))
    np.savez_compressed(os.path.join(HERE, 'beam_options_stub.npz'), **out)


def make_model():
    from modules.tokenizers_new import build_my_tokenizer
    tokenizer = build_my_tokenizer(os.path.join(REF, 'config/tokenizer'), data_name='iu_xray')
    tmp = os.path.join(tempfile.gettempdir(), 'evoke_golden')
    os.makedirs(tmp, exist_ok=True)
    case = CASES[MODEL_BASE]
    inp = make_inputs(case, tokenizer.get_vocab_size())
    out = {}
    for oname, opts in MODEL_OPTS.items():
        args = make_args(tmp, tokenizer, case['max_seq_len'], case['beam_size'], case.get('multiview', True))
        args.update(dict(sample_n=1, group_size=1, temperature=1.0, decoding_constraint=0, output_logsoftmax=1, length_penalty=''))
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
        done = [m.done_beams for m in model.modules() if hasattr(m, 'done_beams')][0]
        beam = case['beam_size']
        out[oname + '/seq'] = seq.numpy().astype(np.int64)
        out[oname + '/scores'] = np.array([[e['p'] for e in done[b][:beam]] for b in range(case['B'])], dtype=np.float64)
        out[oname + '/lens'] = np.array([[e['seq'].shape[0] for e in done[b][:beam]] for b in range(case['B'])], dtype=np.int32)
        lp = logp.detach().float()
        out[oname + '/chosen'] = lp.gather(2, seq.unsqueeze(-1))[..., 0].numpy().astype(np.float32)
        out[oname + '/probe_logp'] = lp[..., PROBE_IDS].numpy().astype(np.float32)
        out[oname + '/texts'] = np.array(texts)
        print(oname, 'seq', tuple(seq.shape), 'scores', np.round(out[oname + '/scores'], 4).tolist())
    np.savez_compressed(os.path.join(HERE, MODEL_BASE + '_opts.npz'), **out)


if __name__ == '__main__':
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    what = sys.argv[1:] or ['stub', 'model']
    if 'stub' in what:
        make_stub()
    if 'model' in what:
        make_model()
