"""CPU tests of the sampling decode route: the restatement (tests/sample_restatement.py, on top of the oracle's decoder step) against the
fixtures the imported reference wrote (tests/golden/make_sample_golden.py), the restatement's own filters against torch's formulation
of CaptionModel.sample_next_word, and the model-level dispatch rule of AttModel._sample (modules/att_model.py:150-153) on stub objects."""
import os

import numpy as np
import pytest
import torch

from oracle import functional as O
from oracle import spec as S
from tests import sample_restatement as SR
from tests.golden.cases import CASES, PROBE_IDS, make_inputs

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
V = 1444

# name -> (case of tests/golden/cases.py that supplies the inputs, options): the table of tests/golden/make_sample_golden.py, restated here
# because that module imports the reference checkout
SAMPLE_CASES = {
    'sample224_greedy': ('beam224', dict(max_seq_len=40, sample_method='greedy', block_trigrams=1)),
    'sample224_n2': ('beam224', dict(max_seq_len=24, sample_method='greedy', block_trigrams=1, sample_n=2)),
    'sample224_constraint': ('beam224', dict(max_seq_len=24, sample_method='greedy', block_trigrams=0, decoding_constraint=1)),
    'sample384_L100': ('beam384_b4_L100', dict(max_seq_len=100, sample_method='greedy', block_trigrams=1)),
}
# positions per row whose top-1 / top-2 margin is below 1.6e-2 (= 2 x the GPU suite's decode tolerance), as measured with the reference
LOW_MARGIN = {'sample224_greedy': [2, 3], 'sample224_n2': [1, 1, 0, 0], 'sample224_constraint': [2, 1], 'sample384_L100': [4, 7]}


def load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def test_sample_case_table_matches_the_generator():
    src = open(os.path.join(GOLDEN, 'make_sample_golden.py')).read()
    ns = {}
    exec(src[src.index('SAMPLE_CASES = {'):src.index('def digest')], ns)
    assert ns['SAMPLE_CASES'] == SAMPLE_CASES


@pytest.mark.parametrize('name', list(SAMPLE_CASES))
def test_sample_fixture_shape_and_margins(name):
    base, opts = SAMPLE_CASES[name]
    g = load(name)
    R, T = CASES[base]['B'] * opts.get('sample_n', 1), opts['max_seq_len']
    assert g['seq'].shape == (R, T) and g['top_ids'].shape == (R, T, 8) and g['probe_logp'].shape == (R, T, len(PROBE_IDS))
    assert not (g['seq'] == V - 1).any()                                  # the untrained network never emits [EOS]
    assert (g['top_ids'][..., 0] == g['seq']).all()                       # greedy: the stored row's arg-max is the emitted word
    low = (g['margin'] < 1.6e-2).sum(1)
    assert low.tolist() == LOW_MARGIN[name]
    assert (low <= 0.1 * T).all()


@pytest.mark.parametrize('name', list(SAMPLE_CASES))
def test_sample_restatement_reproduces_the_reference(name):
    base, opts = SAMPLE_CASES[name]
    case, g = CASES[base], load(name)
    inp = make_inputs(case, V)
    cfg = dict(O.DEFAULT_CFG, **opts)
    P = S.procedural_state(S.finetune_spec(V))
    with torch.no_grad():
        x, m = O.finetune_encoder_states(P, inp['images'], inp['patient_ids'], case['B'], inp['inc_ids'], inp['inc_masks'], cfg, O.Ctx())
        seq, logp = SR.sample(P, x, m, cfg, bos=V - 2, eos=V - 1, pad=0)
    d = SR.digest(seq, logp, PROBE_IDS)
    assert d['seq'].tolist() == g['seq'].tolist()
    assert d['top_ids'].tolist() == g['top_ids'].tolist()
    fin = np.isfinite(g['probe_logp'])
    assert (np.isfinite(d['probe_logp']) == fin).all()                    # (the decoding constraint's -inf column can be a probe)
    e_top = np.abs(d['top_logp'] - g['top_logp']).max()
    e_probe = np.abs(d['probe_logp'][fin] - g['probe_logp'][fin]).max()
    print('[%s] restatement vs reference stored log-probabilities: top-8 %.2e, probes %.2e' % (name, e_top, e_probe))
    assert e_top <= 5e-5 and e_probe <= 5e-5, (e_top, e_probe)
    if name == 'sample224_n2':
        # only the first B of the B * sample_n rows are trigram-blocked: rows 0-1 (both copies of study 0) agree, and so do rows 2-3
        assert d['seq'][0].tolist() == d['seq'][1].tolist() and d['seq'][2].tolist() == d['seq'][3].tolist()


def test_sample_trigram_penalty_holds_counts():
    """(a, b, w) seen once, twice and three times in front of a row that ends in (a, b)"""
    V1 = 32
    logp = torch.zeros(2, V1)
    #            a  b  w1 a  b  w2 a  b  w2 a  b  w3 a  b  w3 a  b  w3 a  b
    hist = [3, 4, 9, 3, 4, 7, 3, 4, 7, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4]
    seq = torch.tensor([hist, hist])
    out = SR.adjust_rows(logp, seq, len(hist), block_rows=1, decoding_constraint=0)
    unit = np.float32(-0.693) * np.float32(2.0)
    assert out[0, 9].item() == unit and out[0, 7].item() == np.float32(2) * np.float32(-0.693) * np.float32(2.0)
    assert out[0, 5].item() == np.float32(3) * np.float32(-0.693) * np.float32(2.0)
    assert out[0].count_nonzero().item() == 3 and out[1].count_nonzero().item() == 0          # block_rows = 1: row 1 is left alone
    out = SR.adjust_rows(logp, seq, len(hist), block_rows=0, decoding_constraint=1)
    assert torch.isinf(out[:, 4]).all() and torch.isfinite(out).sum().item() == 2 * (V1 - 1)


@pytest.mark.parametrize('method', ['top5', 'top0.9', 'top1', 'sample'])
@pytest.mark.parametrize('temperature', [0.7, 1.0])
def test_sample_filter_matches_the_torch_formulation(method, temperature):
    """filter_row against CaptionModel.sample_next_word's own tensor operations (caption_model.py:378-398): same kept set, same
    distribution over it"""
    g = torch.Generator().manual_seed(3)
    code, param = SR.parse_method(method)
    for _ in range(8):
        row = torch.log_softmax(torch.randn(1445, generator=g) * 3.0, 0)
        lp = (row / temperature).unsqueeze(0)
        if code == SR.TOPP:
            probs = torch.softmax(lp, 1)
            sp, si = torch.sort(probs, descending=True, dim=1)
            mask = sp.cumsum(1) < param
            mask = torch.cat([torch.ones_like(mask[:, :1]), mask[:, :-1]], 1)
            sp = sp * mask.float()
            want = torch.zeros_like(probs).scatter_(1, si, sp / sp.sum(1, keepdim=True))[0]
        elif code == SR.TOPK:
            tk, ix = torch.topk(lp, int(param), dim=1)
            want = torch.softmax(torch.full_like(lp, float('-inf')).scatter(1, ix, tk), 1)[0]
        else:
            want = torch.softmax(lp, 1)[0]
        f = SR.filter_row(row, temperature, code, param)
        if f['gap'] < 1e-6:
            continue
        assert (f['kept'] == (want > 0).numpy()).all()
        np.testing.assert_allclose(f['weights'] / f['weights'].sum(), want.double().numpy(), rtol=0, atol=1e-6)
        w, _ = SR.draw(f['weights'], 0.0)
        assert w == int(np.nonzero(f['kept'])[0][0])
        w, _ = SR.draw(f['weights'], 1.0 - 1e-12)
        assert w == int(np.nonzero(f['kept'])[0][-1])


def test_sample_step_finished_rows_emit_pad_and_zero_rows():
    V1, eos, pad = 16, 15, 0
    seq = torch.zeros(3, 4, dtype=torch.long)
    unf = torch.ones(3, dtype=torch.bool)
    lp = torch.full((3, V1), -5.0)
    lp[0, eos] = lp[1, 3] = lp[2, 4] = -0.1
    SR.sample_step(lp, seq, unf, 0, eos, pad, 0, 0, 1.0, SR.GREEDY, 0.0)
    assert unf.tolist() == [False, True, True] and seq[:, 0].tolist() == [eos, 3, 4]
    lp = torch.full((3, V1), -5.0)
    lp[0, 7] = lp[1, eos] = lp[2, 4] = -0.1
    st = SR.sample_step(lp, seq, unf, 1, eos, pad, 0, 1, 1.0, SR.GREEDY, 0.0)
    # row 2: the decoding constraint takes 4 out (4 cannot follow 4), the rest ties at -5 -> the lowest index
    assert seq[:, 1].tolist() == [pad, eos, 0] and unf.tolist() == [False, False, True]
    assert st['stored'][0].abs().sum().item() == 0 and st['stored'][1, eos].item() == pytest.approx(-0.1)


def _route(args):
    from evoke_amd.model_pretrain_finetune import decode_route
    return decode_route(args)


def test_sample_dispatch_rule():
    """att_model.py:150-153: beam_size > 1 with 'greedy' / 'beam_search' -> beam search; group_size > 1 -> diverse sampling (not on the
    path); everything else -> _sample"""
    assert _route(dict(beam_size=3, sample_method='beam_search')) == 'beam'
    assert _route(dict(beam_size=3, sample_method='greedy')) == 'beam'
    assert _route(dict(beam_size=3)) == 'beam'                                     # opt.get('sample_method', 'greedy')
    assert _route(dict(beam_size=1, sample_method='greedy')) == 'sample'
    assert _route(dict(beam_size=1, sample_method='beam_search')) == 'sample'
    assert _route(dict(sample_method='greedy')) == 'sample'                        # opt.get('beam_size', 1)
    assert _route(dict(beam_size=3, sample_method='top5')) == 'sample'
    assert _route(dict(beam_size=3, sample_method='top0.9', sample_n=2)) == 'sample'
    with pytest.raises(NotImplementedError, match='group_size'):
        _route(dict(beam_size=1, sample_method='greedy', group_size=2))
    with pytest.raises(NotImplementedError, match='group_size'):
        _route(dict(beam_size=3, sample_method='top5', group_size=2))
    assert _route(dict(beam_size=3, sample_method='beam_search', group_size=2)) == 'beam'     # (beam_search raises on it, as before)


def test_sample_method_parsing_matches_the_engine():
    from evoke_amd import decode
    for m in ('greedy', 'sample', 'beam_search', 'top5', 'top0.9', 'top1', 'top40.0'):
        assert decode.parse_sample_method(m) == SR.parse_method(m), m
    with pytest.raises(NotImplementedError, match='gumbel'):
        decode.parse_sample_method('gumbel')
