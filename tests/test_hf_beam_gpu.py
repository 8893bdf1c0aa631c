"""GPU tests of the distilgpt2 backend's device-resident beam search (evoke_amd/gpt2_decode.py): evk_hf_beam_step against the step-by-step
restatement, evk_decode_attention_wide against f32 torch and against itself, the per-step log-probabilities of the device step against
the CPU oracle, the whole session under capture and replay, the free-running model, and the serving loop."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.hf_beam_restatement import SCHEDULE, HFBeam, hf_beam_search, synthetic_rows
from tests.helpers import ARGS, GOLDEN, STORE_DTYPE, V, load_tokenizer
from tests.test_hf_beam_cpu import ALL_EARLY, KERNEL_SEED

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16 = os.environ.get('EVK_STORE', 'f16').lower() == 'f16'
BOS, EOS, PAD = V - 2, V - 1, 0
D, LAYERS, HEADS = 2048, 3, 8          # the decoder sizes of the EVOKE YAML files: head size 256


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the bookkeeping kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1, 2, 3, 4, 8])
@pytest.mark.parametrize('Vv,ld', [(37, 40), (1444, 1448)])
def test_hf_beam_step_follows_the_restatement_step_by_step(Vv, ld, nb):
    from evoke_amd import hip as H
    B, max_len, seed, dev = 3, 12, KERNEL_SEED[nb], 'cuda'
    R, bos, eos, pad = B * nb, Vv - 2, Vv - 1, 0
    ref = HFBeam(B, nb, Vv, max_len, bos, eos, pad, anc_cols=12)
    seqs = ref.seqs.clone().to(dev)
    scores = ref.scores.clone().to(dev)
    anc = ref.anc.clone().to(dev)
    words = torch.full((R,), -7, dtype=torch.long, device=dev)
    pos = torch.zeros(1, dtype=torch.long, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    hyp_score = torch.full((B, nb), -float('inf'), dtype=torch.float64, device=dev)
    hyp_len = torch.zeros(B, nb, dtype=torch.int32, device=dev)
    hyp_seq = torch.full((B, nb, max_len), pad, dtype=torch.long, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    n_done = torch.zeros(1, dtype=torch.int32, device=dev)
    for t in range(max_len - 1):
        rows = synthetic_rows(seed, t, R, Vv, eos, nb, SCHEDULE)
        logp = torch.full((R, ld), float('nan'), dtype=torch.float32)          # (a read beyond the V valid columns would show)
        logp[:, :Vv] = rows
        logp = logp.to(dev)
        last = t == max_len - 2
        H.check(H.lib.evk_hf_beam_step(H.ptr(logp), ld, Vv, nb, B, max_len, H.ptr(pos), eos, pad, int(last), H.ptr(scores), H.ptr(seqs), H.ptr(words),
                                       H.ptr(anc), 12, H.ptr(hyp_score), H.ptr(hyp_len), H.ptr(hyp_seq), H.ptr(done), H.ptr(n_done), H.ptr(pos),
                                       H.ptr(ticket), H.stream()), 'hf_beam_step')
        ref.step(rows, force_end=last)
        what = 'V=%d nb=%d step %d' % (Vv, nb, t)
        assert int(pos) == t + 1 == ref.pos, what
        assert torch.equal(words.cpu(), ref.words), what
        assert torch.equal(seqs.cpu(), ref.seqs), what
        assert torch.equal(anc.cpu(), ref.anc), what
        assert torch.equal(scores.cpu().view(torch.int32), ref.scores.view(torch.int32)), what          # bit for bit
        assert done.cpu().tolist() == [int(d) for d in ref.done], what
        assert int(n_done) == sum(ref.done) and int(ticket) == 0, what
    w_score, w_len, w_seq = ref.lists()
    assert torch.equal(hyp_len.cpu(), w_len) and bool((w_len > 0).all())
    assert torch.equal(hyp_seq.cpu(), w_seq)
    assert torch.equal(hyp_score.cpu(), w_score), (hyp_score.cpu(), w_score)          # f64, equal to the restatement's Python floats


# ---------------------------------------------------------------------------------------------------------------------------------
# (f) single-query attention at head sizes 128 / 256
# ---------------------------------------------------------------------------------------------------------------------------------
def _wide(q, ldq, k, v, knew, vnew, mask, rowmap, last_pos, R, S, heads, dh, kv_div):
    from evoke_amd import hip as H
    out = torch.empty(R, 1, heads * dh, dtype=STORE_DTYPE, device='cuda')
    p = lambda t: t if isinstance(t, int) else H.ptr(t)          # noqa: E731
    H.check(H.lib.evk_decode_attention_wide(p(q), ldq, H.ptr(k), H.ptr(v), p(knew), p(vnew), H.ptr(mask), H.ptr(rowmap), H.ptr(last_pos), H.ptr(out),
                                            R, S, heads, dh, kv_div, C.c_float(1.0 / dh ** 0.5), H.stream()), 'decode_attention_wide')
    return out


def _close(got, want, rtol, atol, what):
    got, want = got.detach().float().cpu(), want.detach().float().cpu()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    assert bool((err <= tol).all()), '%s max err %.4g (tol %.4g)' % (what, err.max().item(), tol.flatten()[err.argmax()].item())


@pytest.mark.parametrize('R,S,heads,dh,last,kv_div,masked', [(6, 24, 2, 256, 17, 1, False), (6, 24, 2, 128, 0, 1, False), (5, 256, 1, 256, 255, 1, False),
                                                              (8, 50, 8, 256, None, 4, False), (7, 100, 3, 128, None, 1, True)])
def test_wide_head_single_query_attention(R, S, heads, dh, last, kv_div, masked):
    torch.manual_seed(11)
    BF, HD, dev = STORE_DTYPE, heads * dh, 'cuda'
    Rk = R // kv_div
    q = (torch.randn(R, 1, HD, device=dev) * 0.8).to(BF)
    k = (torch.randn(Rk, S, HD, device=dev) * 0.8).to(BF)
    v = torch.randn(Rk, S, HD, device=dev).to(BF)
    n_live = S if last is None else last + 1
    if last is not None:
        k[:, n_live:] = 3e4          # positions beyond last_pos: any read of them shows
        v[:, n_live:] = 3e4
    last_pos = torch.tensor([last], dtype=torch.long, device=dev) if last is not None else None
    mask = None
    if masked:
        lens = torch.randint(1, S + 1, (Rk,), device=dev)
        mask = (torch.arange(S, device=dev).unsqueeze(0) < lens.unsqueeze(1)).to(torch.uint8).contiguous()
    out = _wide(q, 0, k, v, None, None, mask, None, last_pos, R, S, heads, dh, kv_div)
    qf = q.float().view(R, heads, 1, dh)
    kf = k.float()[:, :n_live].repeat_interleave(kv_div, 0).view(R, n_live, heads, dh).permute(0, 2, 1, 3)
    vf = v.float()[:, :n_live].repeat_interleave(kv_div, 0).view(R, n_live, heads, dh).permute(0, 2, 1, 3)
    sc = (qf @ kf.transpose(-1, -2)) / dh ** 0.5
    if mask is not None:
        sc = sc.masked_fill(mask.repeat_interleave(kv_div, 0).view(R, 1, 1, S) == 0, float('-inf'))
    want = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(R, 1, HD)
    _close(out, want, 1e-2, 1e-2, 'wide decode attention R=%d S=%d dh=%d' % (R, S, dh))          # the 64-wide kernel's bound
    if kv_div > 1:
        # the beams of a study sharing one K / V row: the same bits as repeated rows
        rep = _wide(q, 0, k.repeat_interleave(kv_div, 0).contiguous(), v.repeat_interleave(kv_div, 0).contiguous(), None, None, None, None, last_pos,
                    R, S, heads, dh, 1)
        assert torch.equal(out, rep)
    if last is not None:
        # a row table that sends every earlier position to another row: the same bits as the same call on gathered caches
        # (row r, position s) -> row r + 1 + s mod (R - 1): an offset in 1 .. R - 1, never a multiple of R
        rowmap = ((torch.arange(R, device=dev).view(R, 1) + 1 + torch.arange(S, device=dev).view(1, S) % (R - 1)) % R).to(torch.int32)
        rowmap[:, last:] = torch.arange(R, device=dev, dtype=torch.int32).view(R, 1)
        rowmap = rowmap.contiguous()
        if last > 0 and R > 1:
            assert bool((rowmap[:, :last] != torch.arange(R, device=dev).view(R, 1)).all())
        gi = rowmap.long().unsqueeze(-1).expand(R, S, HD)
        kg, vg = k.gather(0, gi).contiguous(), v.gather(0, gi).contiguous()
        ind = _wide(q, 0, k, v, None, None, None, rowmap, last_pos, R, S, heads, dh, 1)
        gat = _wide(q, 0, kg, vg, None, None, None, None, last_pos, R, S, heads, dh, 1)
        assert torch.equal(ind, gat)
        _close(ind, (torch.softmax((qf @ kg.float()[:, :n_live].view(R, n_live, heads, dh).permute(0, 2, 1, 3).transpose(-1, -2)) / dh ** 0.5, -1)
                     @ vg.float()[:, :n_live].view(R, n_live, heads, dh).permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(R, 1, HD), 1e-2, 1e-2, 'row table')
        # the fused append: outputs and caches bit-identical to write-then-attend, q read in place from the fused q | k | v row
        qkv = torch.cat([q.view(R, HD), k[:, last].contiguous(), v[:, last].contiguous()], dim=1).contiguous()          # (R, 3 HD)
        ka, va = k.clone(), v.clone()
        ka[:, last] = 3e4
        va[:, last] = 3e4
        base = qkv.data_ptr()
        fused = _wide(base, 3 * HD, ka, va, base + 2 * HD, base + 4 * HD, None, rowmap, last_pos, R, S, heads, dh, 1)
        assert torch.equal(fused, ind)
        assert torch.equal(ka, k) and torch.equal(va, v)


# ---------------------------------------------------------------------------------------------------------------------------------
# the decoder of the `gpt2` fixture: 3 layers x 2048 x 8 heads, procedural weights
# ---------------------------------------------------------------------------------------------------------------------------------
def _build_decoder(beam_size=3, max_seq_len=16):
    from evoke_amd.gpt2 import DistilGPT2TextDecoderModel
    from oracle import gpt2 as G, spec as S
    args = dict(ARGS, decoder_hidden_size=D, decoder_num_hidden_layers=LAYERS, decoder_num_attention_heads=HEADS, beam_size=beam_size,
                max_seq_len=max_seq_len)
    dec = DistilGPT2TextDecoderModel(args, load_tokenizer())
    P = S.procedural_state(G.gpt2_spec(V, D, LAYERS))
    sd = {k[len('text_decoder.'):]: v for k, v in P.items()}
    sd['decoder.encoder_decoder.decoder.lm_head.weight'] = sd['decoder.encoder_decoder.decoder.transformer.wte.weight']
    dec.load_state_dict(sd)
    return dec.cuda().eval(), P


def _enc(scale=0.5):
    from oracle import spec as S
    return (S.det((3, 50, D), a=.013, b=.007, c=.3) * scale).to(STORE_DTYPE).cuda()


@pytest.fixture(scope='module')
def decoder():
    from evoke_amd import ops
    dec, P = _build_decoder()
    ops.set_dropout_enabled(False)
    yield dec, P
    ops.set_dropout_enabled(True)


def _configure(dec, beam_size, max_seq_len):
    dec.beam_size, dec.max_seq_len = beam_size, max_seq_len
    return dec


# (g)
def test_device_step_log_probabilities_are_as_close_to_the_oracle_as_the_host_route(decoder):
    """Per-step log-probabilities on one teacher-forced prefix per step (B = 3, S = 50, beam 3, max_seq_len 16): the largest absolute difference
    from the CPU oracle (oracle.gpt2, f32) of the device step's rows and of the host route's logits() + log_softmax on the same prefixes.
    The routes differ only in the attention kernel's accumulation order, so their errors are two draws of the same rounding noise: the device
    figure may be at most 1.5 x the host route's (the spread of a maximum over ~16 x 9 x 1444 entries)."""
    from evoke_amd import gpt2_decode, ops
    from oracle import gpt2 as G
    dec, P = decoder
    _configure(dec, 3, 16)
    nb, B, T = 3, 3, 15
    R = B * nb
    enc = _enc()
    g = torch.Generator().manual_seed(3)
    prefix = torch.randint(1, V - 2, (R, T), generator=g)
    prefix[:, 0] = BOS
    with torch.no_grad():
        encx = enc.float().cpu().repeat_interleave(nb, 0)
        h, _ = G.gpt2_hidden(P, prefix, None, encx, HEADS, LAYERS)
        want = torch.log_softmax(h @ P[G.PRE + 'transformer.wte.weight'].t(), -1)          # (R, T, V)
        # the device step, launch for launch what the captured step issues
        ses = gpt2_decode._GPT2Session(dec, B, nb, 16, enc.shape[1], enc.device)
        ses._refill(enc)
        dev_rows = []
        for t in range(T):
            ses.words.copy_(prefix[:, t].cuda())
            ses.pos.fill_(t)
            ses._step()
            dev_rows.append(ses.logp_buf.clone())
        # the host route
        encg = enc.repeat_interleave(nb, 0).contiguous()
        caches = [dict(k=torch.zeros(R, 16, D, dtype=STORE_DTYPE, device='cuda'), v=torch.zeros(R, 16, D, dtype=STORE_DTYPE, device='cuda'))
                  for _ in range(LAYERS)]
        host_rows = []
        for t in range(T):
            lg = dec.logits(prefix[:, t:t + 1].cuda().contiguous(), None, encg, caches, t)
            host_rows.append(ops.log_softmax(lg.view(R, -1), V))
    dev_err = max(float((dev_rows[t].cpu() - want[:, t]).abs().max()) for t in range(T))
    host_err = max(float((host_rows[t].cpu() - want[:, t]).abs().max()) for t in range(T))
    print('\n[gpt2 step log-probabilities vs oracle] device route %.3e, host route %.3e' % (dev_err, host_err))
    assert dev_err <= 1.5 * host_err, (dev_err, host_err)


# (h)
def _hooked(dec, enc, seed, schedule, nb, n, sync=False):
    """generate() with the step hook replacing the model's rows by the synthetic ones -> (ids, scores), restatement's (ids, scores, trace)"""
    B, R, max_len = enc.shape[0], enc.shape[0] * nb, dec.max_seq_len
    rows = [synthetic_rows(seed, t, R, V, EOS, nb, schedule).cuda() for t in range(max_len - 1)]

    def hook(t, logp, scores):
        if sync:
            torch.cuda.synchronize()
        logp.copy_(rows[t])
    got = dec.generate(enc, num_return_sequences=n, return_scores=True, step_hook=hook)
    want = hf_beam_search(lambda t, s: rows[t].cpu(), B, nb, V, max_len, BOS, EOS, PAD, n=n)
    return got, want


@pytest.mark.parametrize('nb', [3, 8])
def test_session_under_capture_and_replay_equals_the_restatement(decoder, nb):
    dec, _ = decoder
    _configure(dec, nb, 12)
    from evoke_amd import decode
    for n in (1, nb):
        for seed, scale in ((2, 0.5), (3, 0.3)):          # the second call: same session, another batch, another seed -- no state may leak
            (ids, scores), (w_ids, w_scores, _) = _hooked(dec, _enc(scale), seed, SCHEDULE, nb, n)
            what = 'nb=%d n=%d seed=%d' % (nb, n, seed)
            assert ids.dtype == torch.long and ids.shape == w_ids.shape and torch.equal(ids.cpu(), w_ids), what
            assert scores.dtype == torch.float64 and torch.equal(scores.cpu(), w_scores), what
            assert decode.stats['graph'] and decode.stats['gpt2_steps_issued'] == 11, decode.stats


def test_search_stops_issuing_steps_once_every_study_is_done(decoder):
    from evoke_amd import decode, gpt2_decode
    dec, _ = decoder
    _configure(dec, 3, 64)
    enc = _enc()
    (ids, scores), (w_ids, w_scores, trace) = _hooked(dec, enc, 5, ALL_EARLY, 3, 3, sync=True)
    s = min(i for i, t in enumerate(trace) if all(t['done']))
    issued = decode.stats['gpt2_steps_issued']
    print('\n[gpt2 early stop] every study done at step %d, %d steps issued' % (s, issued))
    assert issued <= s + 16
    assert torch.equal(ids.cpu(), w_ids) and torch.equal(scores.cpu(), w_scores)
    gpt2_decode._POLL[0] = False
    try:
        (ids2, scores2), _ = _hooked(dec, enc, 5, ALL_EARLY, 3, 3, sync=True)
        assert decode.stats['gpt2_steps_issued'] == 63
    finally:
        gpt2_decode._POLL[0] = True
    assert torch.equal(ids, ids2) and torch.equal(scores, scores2)


# (i)
def test_free_running_device_search_matches_the_hf_fixture_and_serves_wide_beams(decoder):
    dec, _ = decoder
    enc = _enc()
    _configure(dec, 3, 16)
    assert dec.session_available(enc.shape[1])
    seq = dec.generate(enc).cpu()
    want = torch.from_numpy(np.load(os.path.join(GOLDEN, 'gpt2.npz'))['eval/seq_b3'])
    print('\n   seq hip', seq.tolist())
    print('   seq ref', want.tolist())
    if F16:
        assert seq.shape == want.shape and torch.equal(seq, want)
    _configure(dec, 8, 16)
    ids, scores = dec.generate(enc, num_return_sequences=8, return_scores=True)
    assert ids.shape[0] == 24 and scores.shape == (24,) and bool((ids[:, 0] == BOS).all())
    sc = scores.view(3, 8)
    assert bool(torch.isfinite(sc).all()) and bool((sc[:, 1:] <= sc[:, :-1]).all()), sc


def _child_main():
    """(child process of the test below) the beam-3 search of the fixture decoder on whatever route the environment selects -> JSON"""
    from evoke_amd import ops
    dec, _ = _build_decoder()
    ops.set_dropout_enabled(False)
    print('RESULT ' + json.dumps(dict(session=bool(dec.session_available(50)), seq=dec.generate(_enc()).cpu().tolist())))


def test_host_route_is_kept_behind_its_switch(decoder):
    dec, _ = decoder
    _configure(dec, 3, 16)
    want = dec._generate_host(_enc()).cpu().tolist()
    env = dict(os.environ, EVK_EXPERIMENTAL='1', EVK_GPT2_SESSION='0')
    r = subprocess.run([sys.executable, '-c', 'from tests.test_hf_beam_gpu import _child_main; _child_main()'], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
    assert res['session'] is False and res['seq'] == want


# (j)
def test_serving_loop_runs_the_distilgpt2_backend_in_flight():
    """generate_pipelined over three batches of the ft224_gpt2 case at depth 2 equals forward(mode='inference') batch for batch, also with
    sample_n = beam_size"""
    from evoke_amd import ops
    from evoke_amd.model_pretrain_finetune import FineTune
    from oracle import gpt2 as G, spec as S
    from tests.golden.cases import CASES, make_inputs
    case = CASES['ft224_gpt2']
    inp = make_inputs(case, V)
    args = dict(ARGS, text_decoder='distilgpt2', decoder_hidden_size=D, decoder_num_hidden_layers=LAYERS, decoder_num_attention_heads=HEADS,
                beam_size=case['beam_size'], max_seq_len=case['max_seq_len'])
    model = FineTune(args, load_tokenizer(), 'iu_xray')
    sd = {k: v for k, v in S.procedural_state(S.finetune_spec(V)).items() if not k.startswith('text_decoder.')}
    sd.update(S.procedural_state(G.gpt2_spec(V, D, LAYERS)))
    sd[G.PRE + 'lm_head.weight'] = sd[G.PRE + 'transformer.wte.weight']
    model.load_state_dict(sd, strict=False)
    model = model.cuda().eval()
    ops.set_dropout_enabled(False)
    try:
        assert model.text_decoder.session_available()
        with torch.no_grad():
            b = (inp['images'].cuda(), inp['ids'].cuda(), inp['masks'].cuda(), np.array(inp['patient_ids']), inp['inc_ids'], inp['inc_masks'])
            batches = [b, (b[0] * 1.05,) + b[1:], (b[0] * 0.95,) + b[1:]]
            for n in (1, case['beam_size']):
                model.text_decoder.sample_n = n
                want = [model(*bb, mode='inference') for bb in batches]
                got = list(model.generate_pipelined(batches, mode='inference', depth=2))
                assert len(got) == 3
                for (wt, ws), (gt, gs) in zip(want, got):
                    assert len(wt) == case['B'] * n and ws.shape[0] == case['B'] * n
                    assert wt == gt and torch.equal(ws.cpu(), gs.cpu()), 'generate_pipelined (distilgpt2, sample_n %d) differs from forward' % n
    finally:
        ops.set_dropout_enabled(True)
