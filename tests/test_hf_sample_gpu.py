"""GPU tests of the distilgpt2 backend's sampling route at the model level (evoke_amd/gpt2_decode.py: _GPT2SampleSession behind
DistilGPT2TextDecoderModel.generate): the session under capture and replay against the restatement's token loop on synthetic logits, the
early stop, the launch count against the beam session's, the unchanged defaults, the free-running model against the CPU oracle, the serving
loop, and the refusals.  The decoder is the one tests/test_hf_beam_gpu.py builds."""
import numpy as np
import pytest
import torch

from tests import hf_sample_restatement as HS
from tests.helpers import ARGS, V, load_tokenizer
from tests.test_hf_beam_gpu import BOS, D, EOS, HEADS, LAYERS, PAD, _build_decoder, _enc

pytestmark = pytest.mark.gpu

OPTS = HS.options(do_sample=True, temperature=0.8, top_k=8, top_p=0.9, repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=3)


@pytest.fixture(scope='module')
def decoder():
    from evoke_amd import ops
    dec, P = _build_decoder(beam_size=1, max_seq_len=12)
    ops.set_dropout_enabled(False)
    yield dec, P
    ops.set_dropout_enabled(True)


def _configure(dec, beam_size, max_seq_len):
    dec.beam_size, dec.max_seq_len = beam_size, max_seq_len
    return dec


def synthetic_logits(seed, t, R, finish_by=None):
    """raw logits rows (R, V) of step t: spread 4, and [EOS] far ahead from step 3 + r % 6 on (or from `finish_by` - r % 3)"""
    g = torch.Generator().manual_seed(seed * 1000 + t)
    lg = torch.randn(R, V, generator=g) * 4.0
    for r in range(R):
        if t >= (3 + r % 6 if finish_by is None else finish_by - 1 - r % 3):
            lg[r, EOS] = 60.0
    return lg


def restated(seed, R, max_len, opts, uni, finish_by=None):
    return HS.generate(lambda t, s: synthetic_logits(seed, t, R, finish_by), R, max_len, BOS, EOS, PAD, opts, uni)


def _hooked(dec, enc, seed, n, opts, uni, finish_by=None, sync=False, packed=False):
    """generate() with the step hook replacing the model's logits rows by the synthetic ones"""
    R, max_len = enc.shape[0] * n, dec.max_seq_len
    rows = [synthetic_logits(seed, t, R, finish_by).cuda() for t in range(max_len - 1)]

    def hook(t, logits, scores):
        assert scores is None and tuple(logits.shape) == (R, V) and logits.dtype == torch.float32
        if sync:
            torch.cuda.synchronize()
        logits.copy_(rows[t])
    kw = {k: opts[k] for k in HS.NEUTRAL}
    if packed:
        it = dec.generate(enc, num_return_sequences=n, step_hook=hook, uniforms=uni.cuda(), return_logprobs=True, as_iterator=True, **kw)
        try:
            while True:
                next(it)
        except StopIteration as e:
            return e.value
    return dec.generate(enc, num_return_sequences=n, step_hook=hook, uniforms=uni.cuda(), return_logprobs=True, return_scores=True, **kw)


def _uniforms(seed, R, max_len):
    return torch.rand(R, max_len, generator=torch.Generator().manual_seed(77 + seed))


# (f)
@pytest.mark.parametrize('n', [1, 3])
def test_sampling_session_under_capture_and_replay_equals_the_restatement(decoder, n):
    from evoke_amd import decode
    dec, _ = decoder
    _configure(dec, 1, 12)
    R, max_len = 3 * n, 12
    wants = {}
    for seed in (2, 3):
        uni = _uniforms(seed, R, max_len)
        w = restated(seed, R, max_len, OPTS, uni)
        # the comparison is exact: no decision of the restatement may sit closer to its boundary than f32 sums resolve (inputs and restatement only)
        assert w['min_filter_gap'] > 1e-4 and w['min_draw_gap'] > 1e-5, (seed, w['min_filter_gap'], w['min_draw_gap'])
        assert len(set(w['lengths'].tolist())) > 1
        wants[seed] = (uni, w)
    got = {}
    for graph_on in (True, False):
        decode._GRAPH_ENABLED[0] = graph_on
        try:
            for seed, scale in ((2, 0.5), (3, 0.3)):      # the second call: same session, another batch, another seed -- no state may leak
                uni, w = wants[seed]
                ids, logp, scores = _hooked(dec, _enc(scale), seed, n, OPTS, uni)
                what = 'n=%d seed=%d graph=%s' % (n, seed, graph_on)
                L = min(int(w['lengths'].max()), max_len)
                assert decode.stats['gpt2_route'] == 'sample' and decode.stats['graph'] == graph_on, decode.stats
                assert ids.dtype == torch.long and tuple(ids.shape) == (R, L) and torch.equal(ids.cpu(), w['seqs'][:, :L]), what
                assert logp.dtype == torch.float32 and tuple(logp.shape) == (R, L) and bool((logp[:, 0] == 0).all())
                assert (logp.cpu() - w['tok_logp'][:, :L]).abs().max().item() <= 1e-5, what
                want_sc = w['tok_logp'].double().sum(1) / (w['lengths'] - 1).double()
                assert scores.dtype == torch.float64 and (scores.cpu() - want_sc).abs().max().item() <= 1e-5, what
                packed, logp_full = _hooked(dec, _enc(scale), seed, n, OPTS, uni, packed=True)
                assert torch.equal(packed.cpu(), HS.pack(w['seqs'], w['lengths'])), what
                assert tuple(logp_full.shape) == (R, max_len)
                got[(seed, graph_on)] = (ids.cpu(), logp.cpu())
        finally:
            decode._GRAPH_ENABLED[0] = True
    for seed in (2, 3):                                   # capture / replay and eager issue: the same bits
        assert torch.equal(got[(seed, True)][0], got[(seed, False)][0]) and torch.equal(got[(seed, True)][1], got[(seed, False)][1])


# (g)
def test_sampling_search_stops_issuing_steps_once_every_row_has_finished(decoder):
    from evoke_amd import decode, gpt2_decode
    dec, _ = decoder
    _configure(dec, 1, 64)
    try:
        R, uni = 9, _uniforms(5, 9, 64)
        w = restated(5, R, 64, OPTS, uni, finish_by=5)
        assert w['steps'] is not None and w['steps'] <= 5 and w['min_filter_gap'] > 1e-4 and w['min_draw_gap'] > 1e-5
        ids, logp, _ = _hooked(dec, _enc(), 5, 3, OPTS, uni, finish_by=5, sync=True)
        issued = decode.stats['gpt2_steps_issued']
        print('\n[gpt2 sampling early stop] every row finished at step %d, %d steps issued' % (w['steps'], issued))
        assert issued <= 5 + 16
        L = int(w['lengths'].max())
        assert torch.equal(ids.cpu(), w['seqs'][:, :L])
        gpt2_decode._POLL[0] = False
        try:
            ids2, logp2, _ = _hooked(dec, _enc(), 5, 3, OPTS, uni, finish_by=5, sync=True)
            assert decode.stats['gpt2_steps_issued'] == 63
        finally:
            gpt2_decode._POLL[0] = True
        assert torch.equal(ids, ids2) and torch.equal(logp, logp2)
    finally:
        _configure(dec, 1, 12)


# (h), (i)
def test_sampling_step_needs_no_more_launches_than_the_beam_step_and_defaults_stay_on_the_beam_session(decoder):
    from evoke_amd import decode
    dec, _ = decoder
    enc = _enc()
    _configure(dec, 1, 12)
    neutral = {k: v for k, v in HS.NEUTRAL.items()}
    want = dec.generate(enc)
    assert decode.stats['gpt2_route'] == 'beam'
    beam_launches = decode.stats['step_launches']
    same = dec.generate(enc, **neutral)
    assert decode.stats['gpt2_route'] == 'beam' and torch.equal(want, same)
    dec.generate(enc, do_sample=True, top_k=5, top_p=0.9)
    assert decode.stats['gpt2_route'] == 'sample'
    sample_launches = decode.stats['step_launches']
    print('\n[gpt2 step launches] beam-1 session %s, sampling session %s' % (beam_launches, sample_launches))
    assert beam_launches is not None and sample_launches is not None and sample_launches <= beam_launches
    _configure(dec, 3, 12)
    try:
        want3 = dec.generate(enc, num_return_sequences=3, return_scores=True)
        same3 = dec.generate(enc, num_return_sequences=3, return_scores=True, **neutral)
        assert decode.stats['gpt2_route'] == 'beam' and torch.equal(want3[0], same3[0]) and torch.equal(want3[1], same3[1])
        # (l)
        with pytest.raises(NotImplementedError):
            dec.generate(enc, repetition_penalty=1.2)
    finally:
        _configure(dec, 1, 12)
    with pytest.raises(ValueError, match='uniforms'):
        dec.generate(enc, do_sample=True, uniforms=torch.zeros(3, 12))                   # on the host
    with pytest.raises(ValueError, match='temperature'):
        dec.generate(enc, do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match='num_return_sequences'):
        dec.generate(enc, no_repeat_ngram_size=2, num_return_sequences=2)
    # greedy with a processor: one report per study, no uniforms needed; no id repeats under no_repeat_ngram_size 1
    ids = dec.generate(enc, no_repeat_ngram_size=1, min_length=6).cpu()
    assert ids.shape[0] == 3 and ids.shape[1] >= 6 and bool((ids[:, 0] == BOS).all())
    for row in ids.tolist():
        body = [i for i in row[1:] if i != PAD]
        assert len(body) == len(set(body)) and EOS not in row[:6]


# (j)
def test_free_running_sampling_draws_from_the_top_k_of_the_oracle(decoder):
    from oracle import gpt2 as G
    dec, P = decoder
    _configure(dec, 1, 12)
    enc = _enc()
    R, max_len, k = 3, 12, 5
    uni = _uniforms(11, R, max_len).cuda()
    seen = []

    def hook(t, logits, scores):
        seen.append(logits.clone())
    ids = dec.generate(enc, do_sample=True, top_k=k, uniforms=uni, step_hook=hook).cpu()
    again = dec.generate(enc, do_sample=True, top_k=k, uniforms=uni).cpu()
    assert torch.equal(ids, again)
    other = dec.generate(enc, do_sample=True, top_k=k, uniforms=_uniforms(12, R, max_len).cuda()).cpu()
    assert other.shape != ids.shape or not torch.equal(other, ids)
    L = ids.shape[1]
    with torch.no_grad():
        h, _ = G.gpt2_hidden(P, ids, None, enc.float().cpu(), HEADS, LAYERS)
        want = h @ P[G.PRE + 'transformer.wte.weight'].t()                               # (R, L, V): position t chooses column t + 1
    live = torch.ones(R, L - 1, dtype=torch.bool)                                       # positions whose row had not finished
    for r in range(R):
        row = ids[r].tolist()
        if EOS in row:
            live[r, row.index(EOS):] = False
    err = max(float((seen[t].cpu() - want[:, t])[live[:, t]].abs().max()) for t in range(L - 1) if bool(live[:, t].any()))
    top = torch.topk(want[:, :L - 1], k + 1, dim=-1)
    gap = top.values[..., k - 1] - top.values[..., k]
    sure = live & (gap > 2 * err)
    print('\n[gpt2 sampling vs oracle] top_k %d, device logits within %.3e of the oracle, %d of %d positions compared'
          % (k, err, int(sure.sum()), int(live.sum())))
    assert int(sure.sum()) >= 0.75 * int(live.sum())
    for r in range(R):
        for t in range(L - 1):
            if sure[r, t]:
                assert int(ids[r, t + 1]) in top.indices[r, t, :k].tolist(), (r, t)


# (k)
def test_serving_loop_samples_with_the_configured_generator():
    """generate_pipelined on a FineTune whose args carry do_sample, top_k and a generator returns, batch for batch, what forward returns for
    that batch from the same generator state, with three searches in flight"""
    from evoke_amd import ops
    from evoke_amd.model_pretrain_finetune import FineTune
    from oracle import gpt2 as G, spec as S
    from tests.golden.cases import CASES, make_inputs
    case = CASES['ft224_gpt2']
    inp = make_inputs(case, V)
    gen = torch.Generator(device='cuda')
    args = dict(ARGS, text_decoder='distilgpt2', decoder_hidden_size=D, decoder_num_hidden_layers=LAYERS, decoder_num_attention_heads=HEADS,
                beam_size=1, max_seq_len=case['max_seq_len'], do_sample=True, top_k=5, generator=gen)
    model = FineTune(args, load_tokenizer(), 'iu_xray')
    sd = {k: v for k, v in S.procedural_state(S.finetune_spec(V)).items() if not k.startswith('text_decoder.')}
    sd.update(S.procedural_state(G.gpt2_spec(V, D, LAYERS)))
    sd[G.PRE + 'lm_head.weight'] = sd[G.PRE + 'transformer.wte.weight']
    model.load_state_dict(sd, strict=False)
    model = model.cuda().eval()
    ops.set_dropout_enabled(False)
    try:
        from evoke_amd import decode
        with torch.no_grad():
            b = (inp['images'].cuda(), inp['ids'].cuda(), inp['masks'].cuda(), np.array(inp['patient_ids']), inp['inc_ids'], inp['inc_masks'])
            batches = [b, (b[0] * 1.05,) + b[1:]]
            gen.manual_seed(5)
            want = [model(*bb, mode='inference') for bb in batches]
            assert decode.stats['gpt2_route'] == 'sample'
            gen.manual_seed(5)
            got = list(model.generate_pipelined(batches, mode='inference', depth=3))
            assert len(got) == 2
            for (wt, ws), (gt, gs) in zip(want, got):
                assert len(wt) == case['B'] and wt == gt and torch.equal(ws.cpu(), gs.cpu())
            gen.manual_seed(6)
            other = [model(*bb, mode='inference') for bb in batches]
            assert any(not torch.equal(o[1].cpu(), w[1].cpu()) if o[1].shape == w[1].shape else True for o, w in zip(other, want))
    finally:
        ops.set_dropout_enabled(True)
