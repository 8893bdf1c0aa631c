"""CPU tests of beam search with options (temperature, decoding_constraint, length_penalty, n-best): the restatement
(tests/beam_options_restatement.py) against the fixtures the imported reference wrote (tests/golden/make_golden_beam_options.py), the
fixtures' own properties, and the host-side validation of evoke_amd.decode.beam_search."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import beam_options_restatement as R
from tests.golden.cases import CASES, PROBE_IDS, make_inputs
from tests.helpers import GOLDEN, V

STUB = np.load(os.path.join(GOLDEN, 'beam_options_stub.npz'))
MODEL = np.load(os.path.join(GOLDEN, 'beam224_b4_opts.npz'), allow_pickle=False)
STUB_GEOMS = {'g3x3_L24': dict(B=3, beam=3, max_len=24, V1=23, eos=21), 'g2x4_L16': dict(B=2, beam=4, max_len=16, V1=37, eos=35),
              'g1x4_L2': dict(B=1, beam=4, max_len=2, V1=11, eos=9)}
STUB_OPTS = {'default': {}, 'avg_0': dict(length_penalty='avg_0'), 'wu_0.9': dict(length_penalty='wu_0.9'), 'temp_0.5': dict(temperature=0.5),
             'temp_2': dict(temperature=2.0), 'constraint': dict(decoding_constraint=1),
             'all': dict(length_penalty='wu_0.9', temperature=2.0, decoding_constraint=1)}
MODEL_BASE = 'beam224_b4'
MODEL_OPTS = {'nbest': dict(sample_n=4), 'temp_3': dict(temperature=3.0), 'constraint': dict(decoding_constraint=1),
              'all_wu': dict(sample_n=4, temperature=3.0, decoding_constraint=1, length_penalty='wu_0.9')}
# Which studies of each model option set have EVERY selection margin and every list gap that shapes the output at >= 2 x LOGP_TOL in the
# restatement's trace, i.e. can be pinned free-running on a 16-bit engine: none.  The untrained network's candidates lie close together (the
# smallest selection margins per study are 5.0e-4 / 3.0e-3 for n-best and constraint, 3.3e-4 / 1.4e-4 under temperature 3), as at default
# options (tests/golden/beam224_b4_trace.npz: 5e-4).  By the rule "drop an option set whose studies are all indecisive" no set is left for a
# free-running identity test, so tests/test_beam_options_gpu.py pins these sets teacher-forced instead and keeps the identity rule for
# whatever study a later fixture makes decisive.  test_restatement_equals_the_reference_on_the_model keeps this table honest.
DECISIVE = {'nbest': [False, False], 'temp_3': [False, False], 'constraint': [False, False], 'all_wu': [False, False]}
LOGP_TOL_F16 = 8e-3          # tests/test_model_gpu.py::LOGP_TOL of the default build (that module needs no GPU to import, but is large)


def stub_lists(res, g):
    """beam_search()'s lists in the fixture's layout"""
    B, beam, T = g['B'], g['beam'], g['max_len']
    ids, scores, lens = np.zeros((B, beam, T), dtype=np.int64), np.zeros((B, beam)), np.zeros((B, beam), dtype=np.int32)
    chosen, prev = np.zeros((B, beam, T), dtype=np.float32), np.zeros((B, beam, T), dtype=np.float32)
    for b in range(B):
        assert len(res['done'][b]) == beam
        for k, e in enumerate(res['done'][b]):
            n = e['len']
            ids[b, k, :n], scores[b, k], lens[b, k] = e['seq'].numpy(), e['p'], n
            chosen[b, k, :n] = e['logps'].gather(1, e['seq'].unsqueeze(1))[:, 0].numpy()
            if n > 1:
                prev[b, k, 1:n] = e['logps'][1:].gather(1, e['seq'][:-1].unsqueeze(1))[:, 0].numpy()
    return dict(ids=ids, scores=scores, lens=lens, chosen=chosen, prev=prev)


@pytest.mark.parametrize('oname', list(STUB_OPTS))
@pytest.mark.parametrize('gname', list(STUB_GEOMS))
def test_restatement_equals_the_reference_on_the_stub(gname, oname):
    """CaptionModel.beam_search driven by the table stub vs the restatement over the same table: list ids and lengths exactly, scores
    within f32 rounding of the running sum, the stored rows at the chosen and at the previous word exactly (-inf under the constraint)"""
    g = STUB_GEOMS[gname]
    step = R.table_step(STUB[gname + '/table'], STUB[gname + '/start'])
    got = stub_lists(R.beam_search(step, g['B'], g['beam'], g['max_len'], g['eos'], STUB_OPTS[oname]), g)
    want = {k: STUB['%s/%s/%s' % (gname, oname, k)] for k in got}
    assert np.array_equal(got['ids'], want['ids']) and np.array_equal(got['lens'], want['lens'])
    np.testing.assert_allclose(got['scores'], want['scores'], rtol=2.0 ** -23, atol=0)
    assert np.array_equal(got['chosen'], want['chosen']) and np.array_equal(got['prev'], want['prev'])
    if STUB_OPTS[oname].get('decoding_constraint'):
        live = np.arange(g['max_len'])[None, None, :] < want['lens'][:, :, None]
        live[:, :, 0] = False
        assert np.isneginf(want['prev'][live]).all()


def test_stub_fixture_shows_every_option():
    """the fixture's own properties: hypotheses of several lengths, and every option set changes the n-best list of the long geometries"""
    for gname in ('g3x3_L24', 'g2x4_L16'):
        base = STUB[gname + '/default/ids']
        assert len(np.unique(STUB[gname + '/default/lens'])) >= 3, gname
        for oname in STUB_OPTS:
            if oname != 'default':
                assert not np.array_equal(STUB['%s/%s/ids' % (gname, oname)], base), (gname, oname)
    assert (STUB['g1x4_L2/default/lens'] <= 2).all()


def test_length_penalty_table_is_the_reference_formula():
    from evoke_amd import decode
    assert decode._length_divisors('', 5) is None
    assert decode._length_divisors('avg_0', 3) == [1.0, 2.0, 3.0]
    assert decode._length_divisors('wu_0.9', 3) == [((5 + t) ** 0.9) / ((5 + 1) ** 0.9) for t in (1, 2, 3)]
    assert list(R.length_divisors('wu_0.9', 3)) == decode._length_divisors('wu_0.9', 3)
    for bad in ('wu', 'foo_1', 'avg_x', 'wu_0.9_1'):
        with pytest.raises(ValueError, match='length_penalty'):
            decode._length_divisors(bad, 3)


def test_host_validation_needs_no_device():
    """bad options are refused before anything touches the decoder or the device"""
    from evoke_amd import decode
    from evoke_amd.model_pretrain_finetune import decode_route
    base = dict(beam_size=4, max_seq_len=8)
    for bad, exc, pat in ((dict(length_penalty='harmonic_2'), ValueError, 'length_penalty'), (dict(sample_n=2), ValueError, 'sample_n'),
                          (dict(sample_n=0), ValueError, 'sample_n'), (dict(temperature=0.0), ValueError, 'temperature'),
                          (dict(temperature=-1.0), ValueError, 'temperature'), (dict(group_size=2), NotImplementedError, 'repeat_tensor')):
        with pytest.raises(exc, match=pat):
            decode.beam_search(None, None, None, dict(base, **bad))
    with pytest.raises(NotImplementedError, match='repeat_tensor'):
        decode_route(dict(beam_size=1, group_size=2))
    assert decode.beam_options(dict(base, temperature=1, decoding_constraint=0, length_penalty='', sample_n=1), 4) is None
    assert decode.beam_options(base, 4, return_logprobs=True)['return_logprobs'] is True
    decode._warned.discard('suppress_UNK')
    with pytest.warns(UserWarning, match='suppress_UNK'):
        decode.beam_options(dict(base, suppress_UNK=1), 4)


def test_retired_decode_paths_are_gone():
    """the legacy beam search, the switches that selected lost experiments and the key-mask form of the static step"""
    import inspect
    from evoke_amd import decode
    for name in ('_beam_search_legacy', '_INDIRECT', '_FUSED_BOOK', '_FUSED_APPEND', '_FUSED_LN'):
        assert not hasattr(decode, name), name
    assert 'kmask' not in inspect.signature(decode._DecoderState.step_static).parameters


@functools.lru_cache(maxsize=None)
def model_restatement(oname):
    """the restatement over the oracle's decoder on case beam224_b4 under one option set of the model fixture"""
    from oracle import functional as O, spec as S
    case = CASES[MODEL_BASE]
    opts = MODEL_OPTS[oname]
    inp = make_inputs(case, V)
    cfg = dict(O.DEFAULT_CFG, max_seq_len=case['max_seq_len'], beam_size=case['beam_size'])
    P = S.procedural_state(S.finetune_spec(V))
    with torch.no_grad():
        x, m = _encoder_states(case['B'])
        step = R.model_step(P, x, m, cfg, V - 2, case['beam_size'])
        res = R.beam_search(step, case['B'], case['beam_size'], case['max_seq_len'], V - 1, opts)
    res['out'] = R.output(res, case['B'], case['beam_size'], case['max_seq_len'], opts.get('sample_n', 1))
    return res


@functools.lru_cache(maxsize=None)
def _encoder_states(B):
    from oracle import functional as O, spec as S
    case = CASES[MODEL_BASE]
    inp = make_inputs(case, V)
    cfg = dict(O.DEFAULT_CFG, max_seq_len=case['max_seq_len'], beam_size=case['beam_size'])
    P = S.procedural_state(S.finetune_spec(V))
    return O.finetune_encoder_states(P, inp['images'], inp['patient_ids'], B, inp['inc_ids'], inp['inc_masks'], cfg, O.Ctx())


def decisive_studies(res, sample_n, tol):
    """studies whose every selection and every list rank that shapes the output had a margin of at least 2 x tol in the restatement"""
    gaps = res['rank_gap'][:, :sample_n].min(axis=1)
    return (res['margin'].min(axis=0) >= 2 * tol) & (gaps >= 2 * tol)


@pytest.mark.parametrize('oname', list(MODEL_OPTS))
def test_restatement_equals_the_reference_on_the_model(oname):
    """the reference FineTune on beam224_b4 under each option set vs the restatement over the oracle's decoder: ids and lengths exactly,
    list scores and stored log-probabilities to the oracle's own accuracy; and which studies a 16-bit engine could be pinned on
    free-running (margins >= 2 x LOGP_TOL) is what DECISIVE records"""
    case, opts = CASES[MODEL_BASE], MODEL_OPTS[oname]
    n = opts.get('sample_n', 1)
    res = model_restatement(oname)
    seq, slp, scores, lens = res['out']
    assert np.array_equal(seq.numpy(), MODEL[oname + '/seq'])
    assert np.array_equal(lens.reshape(case['B'], n), MODEL[oname + '/lens'][:, :n])
    np.testing.assert_allclose(scores.reshape(case['B'], n), MODEL[oname + '/scores'][:, :n], atol=2e-3, rtol=0)
    chosen = slp.gather(2, seq.unsqueeze(-1))[..., 0].numpy()
    np.testing.assert_allclose(chosen, MODEL[oname + '/chosen'], atol=2e-4, rtol=0)
    probe, want = slp[..., PROBE_IDS].numpy(), MODEL[oname + '/probe_logp']
    assert np.array_equal(np.isfinite(probe), np.isfinite(want))
    np.testing.assert_allclose(np.where(np.isfinite(want), probe, 0), np.where(np.isfinite(want), want, 0), atol=2e-4, rtol=0)
    dec = decisive_studies(res, n, LOGP_TOL_F16)
    print('\n[%s] smallest selection margin per study %s, list gaps %s -> decisive %s' % (
        oname, np.round(res['margin'].min(axis=0), 4), np.round(res['rank_gap'][:, :n], 4).tolist(), dec.tolist()))
    assert dec.tolist() == DECISIVE[oname]


def test_model_fixture_options_change_the_ids():
    base = np.load(os.path.join(GOLDEN, MODEL_BASE + '.npz'))['eval/seq']
    assert np.array_equal(MODEL['nbest/seq'][::4], base) and len({tuple(r) for r in MODEL['nbest/seq'][:4].tolist()}) == 4
    for oname in ('temp_3', 'constraint'):
        assert not np.array_equal(MODEL[oname + '/seq'], base), oname
