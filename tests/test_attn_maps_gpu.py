"""GPU tests of the cross-attention maps of generated reports (decode.beam_search / decode.sample with return_attention,
FineTune.generate_with_attention) against tests/golden/beam224_b4_attn.npz, written by the imported reference
(tests/golden/make_attn_maps_golden.py).  The decoder is fed the fixture's encoder states cast to the storage type: no trunk runs except
in the model-level test.  Tolerance of the maps: four times what the reference's own maps move by when its decoder runs on 16-bit operands
(the fixture's drift16, per layer), the rule of the log-probability tests; no floor."""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests.golden.cases import CASES, make_inputs
from tests.helpers import ARGS, GOLDEN, STORE_DTYPE, V, load_procedural, load_tokenizer

pytestmark = pytest.mark.gpu

BASE = 'beam224_b4'
BIG = 1000.0
EOS, PAD = V - 1, 0
CASE = CASES[BASE]
BEAM_ARGS = dict(ARGS, max_seq_len=CASE['max_seq_len'], beam_size=CASE['beam_size'])
GREEDY_ARGS = dict(ARGS, beam_size=1, max_seq_len=40, sample_method='greedy', block_trigrams=1)


def _gold(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


@pytest.fixture(scope='module')
def model():
    from evoke_amd.model_pretrain_finetune import FineTune
    from oracle import spec as S
    m = FineTune(dict(BEAM_ARGS), load_tokenizer(), 'iu_xray')
    load_procedural(m, S.finetune_spec(V))
    m.eval()
    return m


@pytest.fixture(scope='module')
def fix():
    g = _gold(BASE + '_attn')
    return {k: g[k] for k in g.files}


@contextlib.contextmanager
def switched(flag, value):
    """a one-element switch of evoke_amd.decode ([bool]) set for the block"""
    old, flag[0] = flag[0], value
    try:
        yield
    finally:
        flag[0] = old


@contextlib.contextmanager
def fed(dec, fix):
    """the decoder's encode() replaced by the fixture's encoder states (unmasked), for the searches inside"""
    enc = torch.from_numpy(fix['enc']).to(device='cuda', dtype=STORE_DTYPE).contiguous()
    dec.encode = lambda states, mask: (enc, None)
    try:
        yield enc
    finally:
        del dec.encode


def _sessions(dec):
    from evoke_amd import decode
    return decode._SESSIONS.get(dec, {})


def _layer_ratio(got, want, drift, what):
    """per layer: max |got - want| over 4 x max(drift16); printed, then held to 1"""
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(axis=(0, 1, 3))
    tol = 4.0 * drift.max(axis=(0, 1, 3)).astype(np.float64)
    print('\n[%s] |map - reference| per layer %s, tolerance 4 x max(drift16) %s, ratio %s (largest weight %.4f)'
          % (what, np.array2string(err, precision=3), np.array2string(tol, precision=3), np.array2string(err / tol, precision=3), want.max()))
    return err, tol


def _forced_hook(B, beam):
    """the teacher-forcing hook of the beam tests (test_model_gpu._beam100), restated: at every position only the reference's selection
    keeps a finite log-probability, with the reference's own running scores"""
    tr = _gold(BASE + '_trace')
    flat = torch.from_numpy(tr['flat']).cuda()            # (T, B, K)
    score = torch.from_numpy(tr['score']).cuda()
    V1 = V + 1

    def forced(t, logp, beam_sum):
        nb = 1 if t == 0 else beam
        parent, word = flat[t] // V1, flat[t] % V1
        rows = parent + torch.arange(B, device='cuda').unsqueeze(1) * nb
        new = torch.full_like(logp, -1e30)
        new[rows[:, :beam], word[:, :beam]] = score[t][:, :beam] - beam_sum[:, :nb].gather(1, parent[:, :beam])
        logp.copy_(new)
    return forced


def test_attn_maps_beam_teacher_forced_along_the_reference(model, fix):
    """the forced search returns the reference ids of every study, and the map of every word agrees with the reference's
    decoder.layers[i].src_attn.attn head mean within 4 x max(drift16) per layer"""
    from evoke_amd import decode
    dec, B, beam, T = model.text_decoder, CASE['B'], CASE['beam_size'], CASE['max_seq_len']
    with fed(dec, fix) as enc:
        seq, att = decode.beam_search(dec, None, None, BEAM_ARGS, step_hook=_forced_hook(B, beam), return_attention=True)
    S = enc.shape[1]
    assert decode.stats.get('fused_bookkeeping'), decode.stats
    assert torch.equal(seq.cpu(), torch.from_numpy(_gold(BASE)['eval/seq'])), 'the forced search does not return the reference ids'
    assert seq.cpu().tolist() == fix['beam/ids'].tolist()
    assert att.dtype == torch.float32 and tuple(att.shape) == (B, T, 3, S)
    att = att.cpu().numpy()
    assert np.abs(att.astype(np.float64).sum(-1) - 1).max() <= (S + 2) * 2.0 ** -23
    err, tol = _layer_ratio(att, fix['beam/maps'], fix['beam/drift16'], 'beam, teacher-forced')
    assert (err <= tol).all(), 'per-layer errors %s beyond %s' % (err, tol)


def test_attn_maps_nbest_rows_follow_each_entry_s_own_ancestry(model, fix):
    """sample_n = beam_size: row b * n + k is the map history followed along entry k's own ancestry -- a torch gather through the finished
    list's row table on the session's history, bit for bit; zeros beyond the entry's length"""
    from evoke_amd import decode
    dec, B, beam, T = model.text_decoder, CASE['B'], CASE['beam_size'], CASE['max_seq_len']
    args = dict(BEAM_ARGS, sample_n=beam)

    def eos_for_one(t, logp, beam_sum):               # one hypothesis of study 1 ends early, so that a short entry is in the list
        if t == 5:
            logp.view(B, -1, logp.shape[-1])[1, 0, EOS] += BIG
    with fed(dec, fix):
        seq, att = decode.beam_search(dec, None, None, args, step_hook=eos_for_one, return_attention=True)
    ses = list(_sessions(dec).values())[-1]
    assert ses.hist_attn is not None and ses.lists.opts['sample_n'] == beam
    hist, anc, ln = ses.hist_attn, ses.lists.anc.long(), ses.lists.len
    S = hist.shape[-1] // 3
    assert tuple(att.shape) == (B * beam, T, 3, S) and tuple(seq.shape) == (B * beam, T)
    t_ix = torch.arange(T, device='cuda').view(1, 1, T).expand(B, beam, T)
    want = hist[t_ix, anc.clamp(0, hist.shape[1] - 1)]                                  # (B, beam, T, 3 * S)
    want = want * (t_ix < ln.unsqueeze(-1)).unsqueeze(-1).to(want.dtype)
    assert torch.equal(att.view(B, beam, T, 3 * S), want)
    assert int(ln.min()) == 6 and int(ln.max()) == T
    short = (ln.view(-1) == 6).nonzero()[0].item()
    assert (att[short, 6:] == 0).all() and (att[short, :6].sum(-1) > 0.99).all() and seq[short, 5].item() == EOS
    # the entries of a study differ in their ancestry: so do their maps
    assert not torch.equal(att[0], att[1])


def test_attn_maps_sampling_route_greedy_forced(model, fix):
    """the sampling route under the fixture's greedy ids: the maps against the reference under the same rule; a row that has emitted
    [EOS] returns zeros from the next position on, the other row's bits unchanged"""
    from evoke_amd import decode
    dec = model.text_decoder
    want = torch.from_numpy(fix['greedy/ids']).cuda()
    R, T = want.shape
    rows = torch.arange(R, device='cuda')

    def forced(t, logp):
        logp[rows, want[:, t]] += BIG

    at = 5

    def forced_eos(t, logp):
        forced(t, logp)
        if t == at:
            logp[1, EOS] += 2 * BIG
    with fed(dec, fix) as enc:
        seq, none, att = decode.sample(dec, None, None, GREEDY_ARGS, step_hook=forced, return_attention=True)
        seq1, _, att1 = decode.sample(dec, None, None, GREEDY_ARGS, step_hook=forced_eos, return_attention=True)
    S = enc.shape[1]
    assert none is None and torch.equal(seq, want) and tuple(att.shape) == (R, T, 3, S) and att.dtype == torch.float32
    err, tol = _layer_ratio(att.cpu().numpy(), fix['greedy/maps'], fix['greedy/drift16'], 'sampling route, greedy, teacher-forced')
    assert seq1[1, at].item() == EOS and (seq1[1, at + 1:] == PAD).all()
    assert (att1[1, at + 1:] == 0).all() and torch.equal(att1[1, :at + 1], att[1, :at + 1]) and torch.equal(att1[0], att[0])
    assert (err <= tol).all(), 'per-layer errors %s beyond %s' % (err, tol)


def test_attn_maps_step_keeps_its_launch_count_and_replays_what_it_issues(model, fix):
    """the maps come out of the cross-attention launch: the captured step of a maps search has the launch count of the same search with
    log-probability rows only, and the replayed step returns the bits of the eagerly issued one"""
    from evoke_amd import decode
    dec = model.text_decoder
    args = dict(BEAM_ARGS, sample_n=CASE['beam_size'])
    with fed(dec, fix):
        seq_g, att_g = decode.beam_search(dec, None, None, args, return_attention=True)
        assert decode.stats.get('graph') and decode.stats.get('replayer'), decode.stats
        n_maps = decode.stats['step_launches']
        decode.beam_search(dec, None, None, args, return_logprobs=True)
        n_logp = decode.stats['step_launches']
        with switched(decode._GRAPH_ENABLED, False):
            seq_e, att_e = decode.beam_search(dec, None, None, args, return_attention=True)
        assert not decode.stats.get('graph')
    print('\n[attn maps] kernel launches of one captured token step: %s with maps, %s with log-probability rows only' % (n_maps, n_logp))
    assert n_maps is not None and n_maps == n_logp
    assert torch.equal(seq_g, seq_e) and torch.equal(att_g, att_e)


def test_attn_maps_do_not_touch_the_plain_search(model, fix):
    """return_attention=False before and after a maps search: the plain session is reused, the ids are what they were, and the two
    searches do not share a session"""
    from evoke_amd import decode
    dec = model.text_decoder
    with fed(dec, fix):
        seq0 = decode.beam_search(dec, None, None, BEAM_ARGS)
        plain = list(_sessions(dec).values())[-1]
        n_plain = decode.stats['step_launches']
        assert plain.lists is None and plain.hist_attn is None and plain.st.maps is None
        seq_m, att = decode.beam_search(dec, None, None, BEAM_ARGS, return_attention=True)
        with_maps = list(_sessions(dec).values())[-1]
        assert with_maps is not plain and with_maps.hist_attn is not None
        seq1 = decode.beam_search(dec, None, None, BEAM_ARGS)
        assert list(_sessions(dec).values())[-1] is plain and decode.stats['step_launches'] == n_plain
    assert torch.equal(seq0, seq1)
    assert isinstance(seq0, torch.Tensor) and tuple(seq_m.shape) == tuple(seq0.shape)


def test_attn_maps_refusals_and_the_model_level_call(model, monkeypatch):
    from evoke_amd import decode
    from evoke_amd.model_pretrain_finetune import FineTune
    dec = model.text_decoder
    inp = make_inputs(CASE, V)
    images, pids = inp['images'].cuda(), np.array(inp['patient_ids'])
    with torch.no_grad():
        texts = model(images, inp['ids'].cuda(), inp['masks'].cuda(), pids, inp['inc_ids'], inp['inc_masks'], mode='sample')[0]
        out = model.generate_with_attention(images, pids)
    B, T = CASE['B'], CASE['max_seq_len']
    assert out['texts'] == texts and tuple(out['ids'].shape) == (B, T)
    S = out['attention'].shape[-1]
    gh, gw = out['grid']
    assert gh * gw == S - 1 and tuple(out['attention'].shape) == (B, T, 3, S)
    glob, patches = decode.attention_grid(out['attention'], out['grid'])
    assert tuple(patches.shape) == (B, T, 3, gh, gw) and (glob == 0).all()            # the decoder never sees the global token
    live = (out['ids'] != PAD)
    assert ((patches.sum((-1, -2)) - 1).abs()[live] < 1e-4).all()
    # -- no session: switched off, or a geometry it does not serve
    with torch.no_grad():
        x, enc_mask = model.encoder_states(images, pids, B)
    with switched(decode._SESSION, False):
        for call in (lambda: decode.beam_search(dec, x, enc_mask, BEAM_ARGS, return_attention=True),
                     lambda: decode.sample(dec, x, enc_mask, GREEDY_ARGS, return_attention=True)):
            with pytest.raises(NotImplementedError, match='EVK_DECODE_SESSION'):
                call()
    monkeypatch.setitem(model.args, 'max_seq_len', 300)
    with pytest.raises(NotImplementedError, match='max_seq_len 300'):
        model.generate_with_attention(images, pids)
    monkeypatch.setitem(model.args, 'max_seq_len', T)
    # -- the distilgpt2 backend
    gpt2 = FineTune(dict(ARGS, text_decoder='distilgpt2', decoder_hidden_size=64, decoder_num_hidden_layers=1, decoder_num_attention_heads=1,
                         beam_size=3, max_seq_len=16), load_tokenizer(), 'iu_xray')
    with pytest.raises(NotImplementedError, match='distilgpt2'):
        gpt2.generate_with_attention(images, pids)
