"""GPU tests of the sampling decode route (evoke_amd.decode.sample, csrc/sample.hip) at model level against the fixtures the imported
reference wrote for AttModel._sample (tests/golden/make_sample_golden.py; default f16-storage build, f32 relational memory).

The engine's decoder runs on 16-bit operands, so its log-probabilities sit within LOGP_TOL of the reference's (the project's flat decode
tolerance, tests/test_model_gpu.py) and a greedy decision can only be pinned where the reference took it with a margin of at least
2 x LOGP_TOL.  Which positions that leaves out is a property of the fixture alone (at most 7 % of a row)."""
import numpy as np
import pytest
import torch

from tests.golden.cases import CASES, PROBE_IDS, make_inputs
from tests.helpers import ARGS, F16_BUILD, V, load_procedural, load_tokenizer
from tests.test_model_gpu import LOGP_TOL
from tests.test_sample_cpu import SAMPLE_CASES, load

pytestmark = pytest.mark.gpu

BIG = 1000.0            # what the teacher-forcing hook adds to the reference's token (and the test takes off the stored row again)
EOS, PAD = V - 1, 0


def _args(name):
    return dict(ARGS, beam_size=1, **SAMPLE_CASES[name][1])


@pytest.fixture(scope='module')
def model():
    from evoke_amd.model_pretrain_finetune import FineTune
    from oracle import spec as S
    m = FineTune(_args('sample224_greedy'), load_tokenizer(), 'iu_xray')
    load_procedural(m, S.finetune_spec(V))
    m.eval()
    return m


_ENC = {}


def _encoder_states(model, base):
    if base not in _ENC:
        case = CASES[base]
        inp = make_inputs(case, V)
        with torch.no_grad():
            _ENC[base] = model.encoder_states(inp['images'].cuda(), np.array(inp['patient_ids']), case['B'], inp['inc_ids'], inp['inc_masks'])
    return _ENC[base]


def _pinned(g):
    """positions whose decision the fixture pins: recorded margin >= 2 x LOGP_TOL"""
    pinned = g['margin'] >= 2 * LOGP_TOL
    if F16_BUILD:
        assert ((~pinned).sum(1) <= 0.1 * pinned.shape[1]).all()          # (the fixture's own property: 7 % in the worst row)
    return pinned


def _first_open(pinned):
    """per row, the first position that is not pinned (T when every position is)"""
    T = pinned.shape[1]
    return [int(np.argmin(row)) if not row.all() else T for row in pinned]


@pytest.mark.parametrize('name', list(SAMPLE_CASES))
def test_sample_teacher_forced_along_the_reference(model, name):
    """the hook makes the reference's token win at every position, so every decoder step sees the reference's prefix: the stored
    log-probabilities at the recorded columns agree to LOGP_TOL, the engine's own arg-max is the reference's token wherever that is pinned,
    and the returned ids are the fixture's (constraint, trigram penalty with block_rows = B, bookkeeping)"""
    from evoke_amd import decode
    g, args = load(name), _args(name)
    want = torch.from_numpy(g['seq'])
    R, T = want.shape
    want_d, rows = want.cuda(), torch.arange(R, device='cuda')

    def forced(t, logp):
        logp[rows, want_d[:, t]] += BIG

    x, enc_mask = _encoder_states(model, SAMPLE_CASES[name][0])
    seq, slp = decode.sample(model.text_decoder, x, enc_mask, args, return_logprobs=True, step_hook=forced)
    assert decode.stats.get('graph') and decode.stats.get('replayer'), decode.stats
    assert torch.equal(seq.cpu(), want), 'the forced run does not return the reference ids'
    slp = slp.cpu()
    assert slp.shape == (R, T, V + 1)
    slp.scatter_add_(2, want.unsqueeze(-1), torch.full((R, T, 1), -BIG))
    top_ids = torch.from_numpy(g['top_ids']).long()
    e_top = (slp.gather(2, top_ids) - torch.from_numpy(g['top_logp'])).abs()
    probe_want = torch.from_numpy(g['probe_logp'])
    probe_got = slp[:, :, PROBE_IDS]
    fin = torch.isfinite(probe_want)
    assert (torch.isfinite(probe_got) == fin).all() and (probe_got[~fin] == probe_want[~fin]).all()      # the constraint's -inf column
    e_probe = torch.where(fin, probe_got - probe_want, torch.zeros_like(probe_got)).abs()
    own = slp.argmax(2)
    pinned = torch.from_numpy(_pinned(g))
    print('\n[%s] teacher-forced |stored logp - reference|: top-8 columns %.2e, probes %.2e (tolerance %.1e); own arg-max equals the reference '
          'token at %s of %d positions per row, %s of them pinned' % (name, e_top.max().item(), e_probe.max().item(), LOGP_TOL,
                                                                     (own == want).sum(1).tolist(), T, pinned.sum(1).tolist()))
    assert e_top.max().item() <= LOGP_TOL and e_probe.max().item() <= LOGP_TOL
    assert (own == want)[pinned].all(), 'the engine prefers another token where the reference margin is %s' % g['margin'][(own != want).numpy() & pinned.numpy()]


@pytest.mark.parametrize('name', list(SAMPLE_CASES))
def test_sample_free_running_follows_the_reference(model, name):
    """ids identical to the reference's up to the first position whose recorded margin is below 2 x LOGP_TOL.  sample224_n2: rows 0-1 (the
    copies of study 0, trigram-blocked) and rows 2-3 (the copies of study 1, which the reference's loop over batch_size leaves unblocked)"""
    from evoke_amd import decode
    g, args = load(name), _args(name)
    want = g['seq']
    x, enc_mask = _encoder_states(model, SAMPLE_CASES[name][0])
    seq, none = decode.sample(model.text_decoder, x, enc_mask, args)
    assert none is None and seq.dtype == torch.long and tuple(seq.shape) == want.shape
    seq = seq.cpu().numpy()
    first = _first_open(_pinned(g))
    print('\n[%s] free-running: identical to the reference for %s positions of %d (first unpinned position per row: %s)'
          % (name, [int((seq[r] == want[r]).cumprod().sum()) for r in range(len(first))], want.shape[1], first))
    for r, p in enumerate(first):
        assert seq[r, :p].tolist() == want[r, :p].tolist(), (name, r)
    if name == 'sample224_n2':
        blocked = load('sample224_greedy')['seq'][:, :want.shape[1]]
        assert want[0].tolist() == want[1].tolist() == blocked[0].tolist()
        assert want[2].tolist() == want[3].tolist() != blocked[1].tolist()                 # study 1 unblocked: another report


@pytest.mark.parametrize('env', [{}, {'EVK_DECODE_THREADS': '1', 'EVK_DECODE_DEPTH': '2', 'EVK_DECODE_BURST': '5'}], ids=['one_thread', 'threads_burst5'])
def test_sample_model_level_beam_size_one(model, env, monkeypatch):
    """FineTune(..., beam_size=1, sample_method='greedy')(mode='inference') takes the sampling route (trigram blocking as configured) and
    generate_pipelined returns what the per-batch call returns, whether this thread issues the token steps or a host thread per search
    issues them in native bursts"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = load('sample224_greedy')
    case = CASES['beam224']
    inp = make_inputs(case, V)
    batch = (inp['images'].cuda(), inp['ids'].cuda(), inp['masks'].cuda(), np.array(inp['patient_ids']), inp['inc_ids'], inp['inc_masks'])
    with torch.no_grad():
        texts, seq = model(*batch, mode='inference')
        piped = list(model.generate_pipelined([batch, batch, batch], mode='inference'))
    seq = seq.cpu()
    assert len(texts) == case['B'] and tuple(seq.shape) == g['seq'].shape
    for r, p in enumerate(_first_open(_pinned(g))):
        assert seq[r, :p].tolist() == g['seq'][r, :p].tolist(), r
    assert len(piped) == 3
    for pt, ps in piped:
        assert pt == texts and torch.equal(ps.cpu(), seq)


def test_sample_eos_rows_continue_as_pad(model):
    """a hook forces [EOS] on row 1 at position 5: [PAD] and zero log-probability rows afterwards, the other row untouched"""
    from evoke_amd import decode
    args = _args('sample224_greedy')
    x, enc_mask = _encoder_states(model, 'beam224')
    at = 5

    def force_eos(t, logp):
        if t == at:
            logp[1, EOS] += BIG

    seq0, slp0 = decode.sample(model.text_decoder, x, enc_mask, args, return_logprobs=True)
    seq1, slp1 = decode.sample(model.text_decoder, x, enc_mask, args, return_logprobs=True, step_hook=force_eos)
    assert torch.equal(seq1[0], seq0[0]) and torch.equal(slp1[0], slp0[0])
    assert torch.equal(seq1[1, :at], seq0[1, :at]) and seq1[1, at].item() == EOS
    assert (seq1[1, at + 1:] == PAD).all() and (slp1[1, at + 1:] == 0).all()
    assert torch.equal(slp1[1, :at], slp0[1, :at]) and slp1[1, at].abs().sum().item() > 0
    assert not (seq0 == EOS).any() and (slp0[:, -1].abs().sum(1) > 0).all()          # the unforced rows run to the last position


def test_sample_stochastic_methods_smoke(model):
    from evoke_amd import decode
    x, enc_mask = _encoder_states(model, 'beam224')
    args = dict(ARGS, beam_size=1, max_seq_len=24, sample_method='top5', temperature=0.7, sample_n=2, block_trigrams=1)
    runs = []
    for seed in (1, 1, 2):
        torch.manual_seed(seed)
        runs.append(decode.sample(model.text_decoder, x, enc_mask, args)[0].cpu())
    assert tuple(runs[0].shape) == (4, 24) and (runs[0] >= 0).all() and (runs[0] <= V).all()
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    assert not torch.equal(runs[0][0], runs[0][1])                                   # the two samples of study 0 draw their own numbers
    u = torch.rand(2, 24, device='cuda')
    a = decode.sample(model.text_decoder, x, enc_mask, dict(args, sample_n=1, sample_method='top0.9'), uniforms=u)[0]
    b = decode.sample(model.text_decoder, x, enc_mask, dict(args, sample_n=1, sample_method='top0.9'), uniforms=u.clone())[0]
    assert torch.equal(a, b)
    greedy, glp = decode.sample(model.text_decoder, x, enc_mask, dict(args, sample_n=1, sample_method='greedy'), return_logprobs=True)
    top1, tlp = decode.sample(model.text_decoder, x, enc_mask, dict(args, sample_n=1, sample_method='top1'), return_logprobs=True)
    assert torch.equal(greedy, top1) and torch.equal(glp, tlp)
    with pytest.raises(NotImplementedError, match='gumbel'):
        decode.sample(model.text_decoder, x, enc_mask, dict(args, sample_method='gumbel'))
    with pytest.raises(NotImplementedError, match='group_size'):
        decode.sample(model.text_decoder, x, enc_mask, dict(args, group_size=2))


def test_sample_eager_fallback_returns_the_same_report(model):
    """geometries without a session (here: the session switched off) run the decoder steps eagerly around the same kernel"""
    from evoke_amd import decode
    g, args = load('sample224_n2'), _args('sample224_n2')
    x, enc_mask = _encoder_states(model, 'beam224')
    saved = decode._SESSION[0]
    decode._SESSION[0] = False
    try:
        seq, slp = decode.sample(model.text_decoder, x, enc_mask, args, return_logprobs=True)
    finally:
        decode._SESSION[0] = saved
    seq = seq.cpu().numpy()
    for r, p in enumerate(_first_open(_pinned(g))):
        assert seq[r, :p].tolist() == g['seq'][r, :p].tolist(), r
    assert tuple(slp.shape) == (4, 24, V + 1)
