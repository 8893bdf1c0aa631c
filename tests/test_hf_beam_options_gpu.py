"""GPU tests of the distilgpt2 backend's beam search with logits processors, length_penalty, early_stopping and num_beams at the model
level (DistilGPT2TextDecoderModel.generate -> gpt2_decode._GPT2BeamOptionsSession): the session under capture and replay and issued eagerly
against the restatement (rows supplied through the step hook), no state or option leak between routes, the early stop, the free-running
model, and the serving loop.  The decoder is tests/test_hf_beam_gpu.py's (3 layers x 2048 x 8 heads)."""
import numpy as np
import pytest
import torch

from tests import hf_beam_options_restatement as R
from tests.hf_beam_restatement import SCHEDULE
from tests.helpers import ARGS, V, load_tokenizer
from tests.test_hf_beam_cpu import ALL_EARLY
from tests.test_hf_beam_gpu import BOS, D, EOS, HEADS, LAYERS, PAD, _build_decoder, _configure, _enc
from tests.test_hf_beam_options_cpu import EARLY_SET, SESSION_SEEDS, SESSION_SETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def decoder():
    from evoke_amd import ops
    dec, _ = _build_decoder()
    ops.set_dropout_enabled(False)
    yield dec
    ops.set_dropout_enabled(True)


def _hooked(dec, enc, seed, schedule, nb, n, opts, sync=False, **kw):
    """generate(num_beams=nb, **opts) with the step hook replacing the model's rows by the sticky ones -> (ids, scores), the restatement's
    (ids, scores, trace)"""
    B, max_len = enc.shape[0], dec.max_seq_len
    rows = [R.sticky_rows(seed, t, B * nb, V, EOS, nb, schedule).cuda() for t in range(max_len - 1)]

    def hook(t, logp, scores):
        if sync:
            torch.cuda.synchronize()
        logp.copy_(rows[t])
    got = dec.generate(enc, num_return_sequences=n, return_scores=True, step_hook=hook, num_beams=nb, **dict(opts, **kw))
    want = R.hf_beam_search_opts(lambda t, s: rows[t].cpu(), B, nb, V, max_len, BOS, EOS, PAD, opts, n=n)
    return got, want


def _plain_step_launches(dec, nb):
    from evoke_amd import decode
    _configure(dec, nb, 12)
    dec.generate(_enc())
    assert decode.stats['gpt2_route'] == 'beam' and decode.stats['graph']
    return decode.stats['step_launches']


@pytest.mark.parametrize('name', sorted(SESSION_SETS))
@pytest.mark.parametrize('nb', [3, 8])
def test_options_session_under_capture_and_replay_and_issued_eagerly_equals_the_restatement(decoder, nb, name):
    from evoke_amd import decode
    dec, opts = decoder, SESSION_SETS[name]
    plain = _plain_step_launches(dec, nb)
    _configure(dec, 2, 12)                                   # beam_size stays at another value: the width is num_beams
    for n in (1, nb):
        for seed, scale in zip(SESSION_SEEDS, (0.5, 0.3)):   # the second call: same session, another batch, another seed -- no state may leak
            (ids, scores), (w_ids, w_scores, _) = _hooked(dec, _enc(scale), seed, SCHEDULE, nb, n, opts)
            what = '%s nb=%d n=%d seed=%d' % (name, nb, n, seed)
            assert ids.dtype == torch.long and ids.shape == w_ids.shape and torch.equal(ids.cpu(), w_ids), what
            assert scores.dtype == torch.float64 and torch.equal(scores.cpu(), w_scores), what
            assert decode.stats['graph'] and decode.stats['gpt2_steps_issued'] == 11 and decode.stats['gpt2_route'] == 'beam-options', decode.stats
            assert decode.stats['step_launches'] == plain, (decode.stats['step_launches'], plain)
            saved = decode._GRAPH_ENABLED[0]
            decode._GRAPH_ENABLED[0] = False                 # the same session, its steps issued eagerly
            try:
                (e_ids, e_scores), _ = _hooked(dec, _enc(scale), seed, SCHEDULE, nb, n, opts)
                assert not decode.stats['graph']
            finally:
                decode._GRAPH_ENABLED[0] = saved
            assert torch.equal(e_ids, ids) and torch.equal(e_scores, scores), what


def test_no_state_or_option_leaks_between_the_routes(decoder):
    from evoke_amd import decode
    dec, enc = decoder, _enc()
    _configure(dec, 3, 12)
    before = dec.generate(enc, num_return_sequences=3, return_scores=True)
    assert decode.stats['gpt2_route'] == 'beam'
    with_opts = dec.generate(enc, num_return_sequences=3, return_scores=True, num_beams=3, no_repeat_ngram_size=2, min_length=8, length_penalty=2.0)
    assert decode.stats['gpt2_route'] == 'beam-options'
    other = dec.generate(enc, num_return_sequences=3, return_scores=True, num_beams=3, repetition_penalty=1.5, early_stopping=True)
    after = dec.generate(enc, num_return_sequences=3, return_scores=True)
    assert decode.stats['gpt2_route'] == 'beam'
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert not (before[0].shape == with_opts[0].shape and torch.equal(before[0], with_opts[0]))
    assert not (other[0].shape == with_opts[0].shape and torch.equal(other[0], with_opts[0]))
    again = dec.generate(enc, num_return_sequences=3, return_scores=True, num_beams=3, no_repeat_ngram_size=2, min_length=8, length_penalty=2.0)
    assert torch.equal(again[0], with_opts[0]) and torch.equal(again[1], with_opts[1])
    # num_beams alone is the plain search at that width, bit for bit, on the plain session
    for k in (3, 5):
        _configure(dec, 2, 12)
        got = dec.generate(enc, num_return_sequences=k, return_scores=True, num_beams=k)
        assert decode.stats['gpt2_route'] == 'beam'
        _configure(dec, k, 12)
        want = dec.generate(enc, num_return_sequences=k, return_scores=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), k


def test_early_stopping_ends_the_search_sooner(decoder):
    from evoke_amd import decode
    dec = decoder
    _configure(dec, 3, 64)
    (ids, scores), (w_ids, w_scores, trace) = _hooked(dec, _enc(), 5, ALL_EARLY, 3, 3, EARLY_SET, sync=True)
    s = min(i for i, t in enumerate(trace) if all(t['done']))
    issued = decode.stats['gpt2_steps_issued']
    print('\n[gpt2 beam options early stop] every study done at step %d, %d steps issued' % (s, issued))
    assert issued <= s + 16
    assert torch.equal(ids.cpu(), w_ids) and torch.equal(scores.cpu(), w_scores)


def test_free_running_model_respects_the_processors(decoder):
    dec = decoder
    _configure(dec, 3, 16)
    ids, scores = dec.generate(_enc(), num_return_sequences=3, return_scores=True, num_beams=3, no_repeat_ngram_size=2, min_length=6)
    ids = ids.cpu()
    assert ids.shape[0] == 9 and bool((ids[:, 0] == BOS).all())
    for row in ids.tolist():
        end = row.index(EOS) + 1 if EOS in row else len(row)
        assert EOS not in row[:6], row                        # no [EOS] before column 6
        grams = list(zip(row[:end], row[1:end]))
        assert len(grams) == len(set(grams)), row             # no repeated bigram
    sc = scores.view(3, 3)
    assert bool(torch.isfinite(sc).all()) and bool((sc[:, 1:] <= sc[:, :-1]).all()), sc


def test_serving_loop_takes_the_options_from_the_configuration():
    """generate_pipelined over three batches of the ft224_gpt2 case with three searches in flight and the configuration keys set equals
    forward(mode='inference') batch for batch, and differs from the plain search"""
    from evoke_amd import decode, ops
    from evoke_amd.model_pretrain_finetune import FineTune
    from oracle import gpt2 as G, spec as S
    from tests.golden.cases import CASES, make_inputs
    case = CASES['ft224_gpt2']
    inp = make_inputs(case, V)
    args = dict(ARGS, text_decoder='distilgpt2', decoder_hidden_size=D, decoder_num_hidden_layers=LAYERS, decoder_num_attention_heads=HEADS,
                beam_size=case['beam_size'], max_seq_len=case['max_seq_len'], num_beams=4, no_repeat_ngram_size=2, min_length=6,
                repetition_penalty=1.2, gpt2_length_penalty=2.0, early_stopping=True)
    model = FineTune(args, load_tokenizer(), 'iu_xray')
    sd = {k: v for k, v in S.procedural_state(S.finetune_spec(V)).items() if not k.startswith('text_decoder.')}
    sd.update(S.procedural_state(G.gpt2_spec(V, D, LAYERS)))
    sd[G.PRE + 'lm_head.weight'] = sd[G.PRE + 'transformer.wte.weight']
    model.load_state_dict(sd, strict=False)
    model = model.cuda().eval()
    ops.set_dropout_enabled(False)
    try:
        with torch.no_grad():
            b = (inp['images'].cuda(), inp['ids'].cuda(), inp['masks'].cuda(), np.array(inp['patient_ids']), inp['inc_ids'], inp['inc_masks'])
            batches = [b, (b[0] * 1.05,) + b[1:], (b[0] * 0.95,) + b[1:]]
            want = [model(*bb, mode='inference') for bb in batches]
            assert decode.stats['gpt2_route'] == 'beam-options'
            got = list(model.generate_pipelined(batches, mode='inference', depth=3))
            assert len(got) == 3
            for (wt, ws), (gt, gs) in zip(want, got):
                assert wt == gt and torch.equal(ws.cpu(), gs.cpu()), 'generate_pipelined (distilgpt2, beam options) differs from forward'
                assert ws.shape[0] == case['B']
    finally:
        ops.set_dropout_enabled(True)
