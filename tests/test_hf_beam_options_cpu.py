"""CPU tests of the distilgpt2 backend's beam search with logits processors, length_penalty, early_stopping and num_beams: the generalised
restatement (tests/hf_beam_options_restatement.py) against what the installed Hugging Face `generate` recorded
(tests/golden/hf_beam_options_tiny.npz, written by tests/golden/make_hf_beam_options_golden.py), the processors and the scorer on hand-made
rows, the preconditions of the GPU tests (the sticky rows make every processor bite), and what needs no device: the keyword checks and
routing of generate(), the export of evk_hf_beam_step_opts and its argument refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import hf_beam_options_restatement as R
from tests.hf_beam_restatement import SCHEDULE, HFBeam
from tests.test_hf_beam_cpu import ALL_EARLY, _decoder, _pad_after_eos

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('repetition_penalty', 'no_repeat_ngram_size', 'min_length', 'length_penalty', 'early_stopping')

# ---- what the GPU tests run (tests/test_hf_beam_options_ops.py, tests/test_hf_beam_options_gpu.py)
# the option sets of the kernel test: each processor alone, rp < 1 with g = 1, everything on
KERNEL_SETS = dict(rp=dict(repetition_penalty=1.3), ngram=dict(no_repeat_ngram_size=2), minlen=dict(min_length=5),
                   rp_lt1_g1=dict(repetition_penalty=0.8, no_repeat_ngram_size=1),
                   all=dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=5, length_penalty=0.5, early_stopping=True))
# (seed, boost, n_sticky) of sticky_rows per (V, nb): the generator's defaults except at one beam, where two candidates per study leave
# little room -- there fewer sticky ids (and at V = 37 a smaller boost) let the [EOS] and the penalised ids reach the candidates
KERNEL_ROWS = {(V, nb): (2, None, 3) for V in (37, 1444) for nb in (1, 2, 3, 4, 8)}
KERNEL_ROWS.update({(37, 1): (11, 4.0, 2), (1444, 1): (2, None, 2)})
SESSION_SETS = dict(processors=dict(repetition_penalty=1.2, no_repeat_ngram_size=2, min_length=5, length_penalty=2.0), all=KERNEL_SETS['all'])
SESSION_SEEDS = (2, 3)
EARLY_SET = dict(early_stopping=True, no_repeat_ngram_size=2)          # the early-stop test: beam 3, max_seq_len 64, seed 5, ALL_EARLY


def kernel_rows(V, nb, t, B=3):
    seed, boost, ns = KERNEL_ROWS[(V, nb)]
    return R.sticky_rows(seed, t, B * nb, V, V - 1, nb, SCHEDULE, boost, ns)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recorded fixture
# ---------------------------------------------------------------------------------------------------------------------------------
def _fixture():
    from oracle import gpt2 as G
    base = np.load(os.path.join(GOLDEN, 'hf_beam_tiny.npz'))
    gold = np.load(os.path.join(GOLDEN, 'hf_beam_options_tiny.npz'))
    V, D, layers, heads, B, S, bos, eos, pad = [int(v) for v in base['dims']]
    sets = [dict(zip(KEYS, (float(o[0]), int(o[1]), int(o[2]), float(o[3]), bool(o[4])))) for o in gold['option_sets']]
    models = {}
    for seed in (0, 1):
        P = {G.PRE + k[len('w%d/' % seed):]: torch.from_numpy(base[k]) for k in base.files if k.startswith('w%d/' % seed)}
        models[seed] = (P, torch.from_numpy(base['enc%d' % seed]))
    memo = {}

    def logp_fn_for(seed, off, nb):
        P, enc = models[seed]

        def logp_fn(step, rows):
            # (the same prefixes come back for every option set and done test of a model: computed once)
            key = (seed, off, nb, step, rows[:, :step + 1].numpy().tobytes())
            if key not in memo:
                h, _ = G.gpt2_hidden(P, rows[:, :step + 1], None, enc.repeat_interleave(nb, 0), heads, layers)
                lg = h[:, -1] @ P[G.PRE + 'transformer.wte.weight'].t()
                lg[:, eos] += float(off)
                memo[key] = torch.log_softmax(lg, -1)
            return memo[key]
        return logp_fn
    cases = []
    for name in (str(c) for c in gold['cases']):
        seed, off, nb, k = [int(tok.lstrip('sonbk_')) for tok in name.split('_')]
        cases.append((name, seed, off, nb, k, torch.from_numpy(gold['case/%s/seq' % name]).long(), torch.from_numpy(gold['case/%s/score' % name])))
    return dict(V=V, B=B, bos=bos, eos=eos, pad=pad, ml=int(gold['max_length'])), sets, cases, logp_fn_for


def test_restatement_reproduces_the_recorded_hf_generate_with_options():
    """With the later release's done test ('running') EVERY recorded case in full -- every sequence of every n-best list, scores within 1e-5
    (the recorder's margin: ~1e-6 per token between HF's and the oracle's log-probabilities over 11 tokens; measured 5.7e-6).  With the
    classic done test, which the kernel follows, every case whose trace shows that the two tests never disagree, in full: at least 64 of
    them, every early_stopping=True case among them.  Each of the eight option sets changes the result of at least one case against the
    same case with neutral options.  At most 6 of the 128 cases of the grid may have been dropped by the recorder."""
    d, sets, cases, logp_fn_for = _fixture()
    V, B, bos, eos, pad, ml = d['V'], d['B'], d['bos'], d['eos'], d['pad'], d['ml']
    assert len(sets) == 8 and 122 <= len(cases) <= 128, len(cases)
    worst, agree, bites = 0.0, [], set()
    neutral = {}
    for name, seed, off, nb, k, want, want_sc in cases:
        fn, opts = logp_fn_for(seed, off, nb), sets[k - 1]
        seqs, scores, _ = R.hf_beam_search_opts(fn, B, nb, V, ml, bos, eos, pad, opts, n=nb, done_test='running')
        assert seqs.shape[0] == want.shape[0] == B * nb, name
        assert torch.equal(_pad_after_eos(seqs, eos, pad, ml), _pad_after_eos(want, eos, pad, ml)), name
        err = float((scores - want_sc).abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (name, err)
        c_seqs, c_scores, tr = R.hf_beam_search_opts(fn, B, nb, V, ml, bos, eos, pad, opts, n=nb, done_test='candidate')
        if sum(t['later_hf_differs'] for t in tr) == 0:
            agree.append(name)
            assert c_seqs.shape == seqs.shape and torch.equal(c_seqs, seqs) and torch.equal(c_scores, scores), name
        if (seed, off, nb) not in neutral:
            neutral[(seed, off, nb)] = R.hf_beam_search_opts(fn, B, nb, V, ml, bos, eos, pad, R.options(), n=nb, done_test='running')[:2]
        n_seqs, n_scores = neutral[(seed, off, nb)]
        if not (torch.equal(_pad_after_eos(n_seqs, eos, pad, ml), _pad_after_eos(want, eos, pad, ml)) and float((n_scores - want_sc).abs().max()) <= 1e-5):
            bites.add(k)
    print('\n[hf beam options fixture] %d cases in full, largest score difference %.2e; the two done tests agree throughout in %d'
          % (len(cases), worst, len(agree)))
    assert len(agree) >= 64, len(agree)
    assert all(name in agree for name, _, _, _, k, _, _ in cases if sets[k - 1]['early_stopping'])
    assert bites == set(range(1, 9)), bites


def test_neutral_options_are_the_plain_restatement():
    """HFBeamOpts with neutral options is HFBeam: state, lists and scores bit for bit"""
    B, nb, V, ml = 3, 3, 37, 12
    a, b = HFBeam(B, nb, V, ml, V - 2, V - 1, 0, anc_cols=12), R.HFBeamOpts(B, nb, V, ml, V - 2, V - 1, 0, anc_cols=12)
    for t in range(ml - 1):
        rows = kernel_rows(V, nb, t)
        a.step(rows, force_end=t == ml - 2)
        b.step(rows, force_end=t == ml - 2)
        assert torch.equal(a.seqs, b.seqs) and torch.equal(a.scores, b.scores) and torch.equal(a.anc, b.anc) and a.done == b.done
    for x, y in zip(a.lists(), b.lists()):
        assert torch.equal(torch.nan_to_num(x.double()), torch.nan_to_num(y.double()))


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-made rows, one processor at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def _rows(B, nb, V, fill=-5.0):
    return torch.full((B * nb, V), fill, dtype=torch.float32)


def _state(hist, V=8, opts=None, nb=1):
    """one study, nb beams, every beam with the history `hist` (ids after [BOS] = V - 2)"""
    st = R.HFBeamOpts(1, nb, V, 10, V - 2, V - 1, 0, opts)
    for c, w in enumerate(hist):
        st.seqs[:, c + 1] = w
    st.pos = len(hist)
    return st


def test_processors_one_by_one_on_hand_made_rows():
    V, eos, bos = 8, 7, 6
    x = torch.tensor([[-1.0, -2.0, -3.0, -0.5, -4.0, -2.5, -6.0, -3.5]])
    # a duplicate id in the history is penalised once; [BOS] is part of the history
    st = _state([1, 3, 1], opts=dict(repetition_penalty=2.0))
    st.step(x.clone())
    assert st.rows[0].tolist() == [-1.0, -4.0, -3.0, -1.0, -4.0, -2.5, -12.0, -3.5]
    # rp < 1 raises a log-probability (negative values are MULTIPLIED)
    st = _state([1, 3, 1], opts=dict(repetition_penalty=0.5))
    st.step(x.clone())
    assert st.rows[0].tolist() == [-1.0, -1.0, -3.0, -0.25, -4.0, -2.5, -3.0, -3.5]
    # a ban and a penalty on the same id: -inf
    st = _state([1, 3, 1], opts=dict(repetition_penalty=2.0, no_repeat_ngram_size=2))
    st.step(x.clone())
    assert st.rows[0, 3] == float('-inf') and st.rows[0, 1] == -4.0          # (1, 3) was seen: 3 is banned after 1
    # g = 1 bans every id present, [BOS] included
    st = _state([1, 3, 1], opts=dict(no_repeat_ngram_size=1))
    st.step(x.clone())
    assert torch.isinf(st.rows[0]).tolist() == [False, True, False, True, False, False, True, False]
    # cur_len = g - 1: no ban; cur_len = g: the first ban
    st = _state([1], opts=dict(no_repeat_ngram_size=3))           # ids: [BOS] 1 -> cur_len 2
    st.step(x.clone())
    assert bool(torch.isfinite(st.rows[0]).all())
    st = _state([1, 6], V=8, opts=dict(no_repeat_ngram_size=3))     # ids: [BOS] 1 [BOS] -> cur_len 3, the one window is the history itself
    st.step(x.clone())
    assert bool(torch.isfinite(st.rows[0]).all())
    st = _state([6, 6], V=8, opts=dict(no_repeat_ngram_size=3))     # [BOS] [BOS] [BOS]: the window bans its own last id
    st.step(x.clone())
    assert torch.isinf(st.rows[0]).tolist() == [False] * 6 + [True, False]
    # min_length at its boundary: cur_len 3 < 4 bans, cur_len 4 does not
    st = _state([1, 2], opts=dict(min_length=4))
    st.step(x.clone())
    assert st.rows[0, eos] == float('-inf')
    st = _state([1, 2, 3], opts=dict(min_length=4))
    st.step(x.clone())
    assert st.rows[0, eos] == -3.5
    # every beam is processed from its OWN history
    st = _state([1], nb=2, opts=dict(no_repeat_ngram_size=1))
    st.seqs[1, 1] = 2
    st.step(torch.cat([x, x]).clone())
    assert st.rows[0, 1] == float('-inf') and st.rows[0, 2] == -3.0 and st.rows[1, 2] == float('-inf') and st.rows[1, 1] == -2.0


def test_length_penalty_reorders_a_list_and_early_stopping_closes_it():
    """a short hypothesis with sum -2 at cur_len 1 and a long one with sum -3 at cur_len 3: sum / cur_len ** lp"""
    V, eos = 8, 7
    order = {}
    for lp in (0.0, 1.0, 2.0):
        st = R.HFBeamOpts(1, 2, V, 10, V - 2, V - 1, 0, dict(length_penalty=lp))
        x = _rows(1, 2, V, -20.0)
        x[0, eos], x[0, 1], x[0, 2] = -2.0, -0.25, -4.0
        st.step(x)                       # ranks: 1 (-0.25), [EOS] (-2.0) -> hypothesis A = sum -2 at cur_len 1; beams: 1, 2
        x = _rows(1, 2, V, -20.0)
        x[0, 3], x[0, 4] = -0.25, -0.5
        st.step(x)                       # cur_len 2: no [EOS]
        x = _rows(1, 2, V, -20.0)
        x[0, eos], x[0, 5] = -2.5, -0.25  # beam 0 sum -0.5: [EOS] candidate -3.0 at rank 1 -> hypothesis B = sum -3 at cur_len 3
        st.step(x)
        sc, ln, _ = st.lists()
        assert sorted(ln[0].tolist()) == [2, 4]
        order[lp] = ln[0].tolist()
        a, b = -2.0 / 1.0 ** lp, -3.0 / 3.0 ** lp
        assert sorted(sc[0].tolist(), reverse=True) == sorted([a, b], reverse=True)
    assert order[0.0] == [2, 4] and order[1.0] == [4, 2] and order[2.0] == [4, 2]          # -2 > -3;  -1 > -2;  -1/3 > -2
    # early_stopping: done as soon as the list is full, whatever the best candidate promises
    done = {}
    for es in (False, True):
        st = R.HFBeamOpts(1, 1, V, 10, V - 2, V - 1, 0, dict(early_stopping=es, length_penalty=2.0))
        x = _rows(1, 1, V, -20.0)
        x[0, eos], x[0, 1] = -0.5, -0.6
        st.step(x)                       # hypothesis -0.5; the best candidate is that same [EOS]: done either way under the classic test
        done[es] = list(st.done)
        st2 = R.HFBeamOpts(1, 2, V, 10, V - 2, V - 1, 0, dict(early_stopping=es))
        x = _rows(1, 2, V, -20.0)
        x[0, 1], x[0, eos], x[0, 2] = -0.1, -3.0, -3.5
        st2.step(x)                      # one hypothesis, list of 2 not full
        x = _rows(1, 2, V, -20.0)
        x[0, 1], x[0, eos], x[0, 2] = -0.1, -6.0, -7.0          # [EOS] of beam 0: sum -6.1 / 2 = -3.05 < -3.0: list full, best candidate -0.2 / 2
        st2.step(x)
        done[(es, 2)] = list(st2.done)
    assert done[False] == [True] and done[True] == [True]
    assert done[(False, 2)] == [False] and done[(True, 2)] == [True]


def test_length_divisors_are_python_powers():
    from evoke_amd import gpt2_decode
    for lp in (0.0, 0.5, 1.0, 2.0, -1.0):
        d = gpt2_decode.length_divisors(lp, 12)
        assert len(d) == 13 and d[1:] == [float(c) ** lp for c in range(1, 13)]
        assert d[1:] == R.length_divisors(lp, 12)[1:]


# ---------------------------------------------------------------------------------------------------------------------------------
# preconditions of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
def _bites(fn, B, nb, V, ml, opts, what):
    """every switched-on processor changes the candidate set of some live study at >= 3 steps; the final lists differ from the neutral
    search's; every live study always has >= 2 * nb finite candidates, and no tie among the candidates that matter"""
    o = R.options(**opts)
    tr = R.hf_beam_search_opts(fn, B, nb, V, ml, V - 2, V - 1, 0, o, n=nb, stop_when_done=False)[2]
    for k in R.PROCESSORS:
        if o[k] != R.NEUTRAL[k]:
            assert sum(1 for t in tr if t['changed'][k] > 0) >= 3, (what, k, [t['changed'] for t in tr])
    assert min(t['finite'] for t in tr if t['live']) >= 2 * nb, what
    assert min(t['min_gap'] for t in tr if t['live']) > 0, what
    a = R.hf_beam_search_opts(fn, B, nb, V, ml, V - 2, V - 1, 0, o, n=nb)
    b = R.hf_beam_search_opts(fn, B, nb, V, ml, V - 2, V - 1, 0, R.options(), n=nb)
    assert not (a[0].shape == b[0].shape and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), what
    return tr


@pytest.mark.parametrize('name', sorted(KERNEL_SETS))
@pytest.mark.parametrize('nb', [1, 2, 3, 4, 8])
@pytest.mark.parametrize('V', [37, 1444])
def test_sticky_rows_make_every_processor_bite_in_the_kernel_cases(V, nb, name):
    _bites(lambda t, s: kernel_rows(V, nb, t), 3, nb, V, 12, KERNEL_SETS[name], (V, nb, name))


@pytest.mark.parametrize('name', sorted(SESSION_SETS))
@pytest.mark.parametrize('seed', SESSION_SEEDS)
@pytest.mark.parametrize('nb', [3, 8])
def test_sticky_rows_make_every_processor_bite_in_the_session_cases(nb, seed, name):
    V = 1444
    _bites(lambda t, s: R.sticky_rows(seed, t, 3 * nb, V, V - 1, nb, SCHEDULE), 3, nb, V, 12, SESSION_SETS[name], (nb, seed, name))


def test_precondition_of_the_gpu_early_stop_test_early_stopping_ends_every_study_sooner():
    """beam 3, max_seq_len 64, seed 5, ALL_EARLY, sticky rows: with early_stopping every study is done at an earlier step than without"""
    V, nb = 1444, 3
    first = {}
    for es in (False, True):
        o = R.options(**dict(EARLY_SET, early_stopping=es))
        tr = R.hf_beam_search_opts(lambda t, s: R.sticky_rows(5, t, 3 * nb, V, V - 1, nb, ALL_EARLY), 3, nb, V, 64, V - 2, V - 1, 0, o, n=nb,
                                   stop_when_done=False)[2]
        first[es] = min(i for i, t in enumerate(tr) if all(t['done']))
    assert first[True] < first[False] and first[True] <= 12, first


# ---------------------------------------------------------------------------------------------------------------------------------
# without a device: keywords, routing, export, argument refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_checks_the_beam_controls_before_it_touches_the_device():
    enc = torch.zeros(2, 5, 64)
    dec = _decoder(beam_size=3)
    for kw, word in ((dict(num_beams=0), 'num_beams'), (dict(num_beams=9), '9'), (dict(early_stopping='never'), 'never'),
                     (dict(early_stopping=2), 'early_stopping'), (dict(length_penalty=float('nan')), 'length_penalty'),
                     (dict(length_penalty='wu_0.9'), 'length_penalty'), (dict(num_beams=2, num_return_sequences=3), 'num_return_sequences'),
                     (dict(num_beams=4, num_return_sequences=0), 'num_return_sequences'), (dict(num_beams=3, repetition_penalty=0.0), 'repetition_penalty'),
                     (dict(num_beams=3, no_repeat_ngram_size=9), '9'), (dict(length_penalty=2.0, min_length=-1), 'min_length'),
                     (dict(num_beams=3, uniforms=torch.zeros(6, 12)), 'uniforms')):
        with pytest.raises(ValueError, match=re.escape(word)):
            dec.generate(enc, **kw)
    for kw, word in ((dict(num_beams=3, do_sample=True), 'do_sample'), (dict(early_stopping=True, do_sample=True, top_k=5), 'do_sample'),
                     (dict(num_beams=1, do_sample=True), 'do_sample'), (dict(num_beams=3, return_logprobs=True), 'return_logprobs'),
                     (dict(length_penalty=0.5, return_logprobs=True), 'return_logprobs')):
        with pytest.raises(NotImplementedError, match=word):
            dec.generate(enc, **kw)
    with pytest.raises(ValueError, match='never'):
        _decoder(beam_size=3, early_stopping='never').generate(enc)
    with pytest.raises(ValueError, match='num_beams'):
        _decoder(beam_size=3, num_beams=12).generate(enc)


def test_routing_rule_of_the_beam_controls():
    """no beam control given: generate() is what it was, the two pinned refusals included; any control given: the beam-options route"""
    enc = torch.zeros(2, 5, 64)
    dec = _decoder(beam_size=3)
    assert dec._beam_controls(None, None, None) is None
    assert dec._beam_controls(None, 1.0, False) is None
    assert dec._beam_controls(None, 1, 0) is None
    assert dec._beam_controls(4, None, None) == dict(num_beams=4, length_penalty=1.0, early_stopping=False)
    assert dec._beam_controls(None, 2.0, None) == dict(num_beams=3, length_penalty=2.0, early_stopping=False)           # width: beam_size
    assert dec._beam_controls(None, None, True) == dict(num_beams=3, length_penalty=1.0, early_stopping=True)
    cfg = _decoder(beam_size=3, num_beams=5, gpt2_length_penalty=0.5, early_stopping=True)
    assert cfg._beam_controls(None, None, None) == dict(num_beams=5, length_penalty=0.5, early_stopping=True)
    assert cfg._beam_controls(2, 1.0, False) == dict(num_beams=2, length_penalty=1.0, early_stopping=False)             # keywords win
    assert _decoder(beam_size=3, length_penalty='wu_0.9')._beam_controls(None, None, None) is None                      # the R2Gen decoder's key
    # the refusals pinned by tests/test_hf_sample_cpu.py, unchanged
    with pytest.raises(NotImplementedError, match='beam_size 1'):
        dec.generate(enc, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match='beam_size 1'):
        _decoder(beam_size=3, do_sample=True, top_k=5).generate(enc)
    with pytest.raises(NotImplementedError, match='needs do_sample or a logits processor'):
        dec.generate(enc, return_logprobs=True)
    assert dec._generation_options(None, None, None, None, None, None, None) is None          # seven positional parameters
    # the options route reaches the device session: here (no GPU) it fails only there, after every check has passed
    seen = {}
    from evoke_amd import gpt2_decode
    real = gpt2_decode.search

    def spy(d, e, n, *a, **kw):
        seen.update(n=n, **kw)
        return 'searched'
    gpt2_decode.search = spy
    try:
        dec.max_seq_len = 12
        assert dec.generate(enc, num_beams=2, repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=4, num_return_sequences=2) == 'searched'
        assert seen == dict(n=2, nb=2, opts=dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_length=4, length_penalty=1.0, early_stopping=False))
        assert cfg.generate(enc, temperature=0.7, top_k=5) == 'searched'                      # warpers without do_sample: inert, as in HF
        assert seen == dict(n=1, nb=5, opts=dict(gpt2_decode.BEAM_NEUTRAL, length_penalty=0.5, early_stopping=True))
        assert dec.generate(enc, num_beams=4) == 'searched' and seen['opts'] == gpt2_decode.BEAM_NEUTRAL and seen['nb'] == 4
    finally:
        gpt2_decode.search = real


def test_library_exports_the_hf_beam_step_opts_and_refuses_bad_arguments():
    from evoke_amd import build, hip as H
    path = build.build()
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'evoke_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+evk_hf_beam_step_opts\s*\(', txt)
    for lib_path in (path, build.LIB_BF16):
        assert hasattr(ctypes.CDLL(lib_path), 'evk_hf_beam_step_opts'), lib_path
    L = H.lib

    def beam(nb=3, V=40, ld=40, rp=1.2, g=2, ml=4):
        return L.evk_hf_beam_step_opts(None, ld, V, nb, 3, 12, None, V - 1, 0, 0, None, None, None, None, 12, None, None, None, None, None, None,
                                       None, ctypes.c_float(rp), g, ml, None, 0, None)
    assert beam(rp=0.0) == -1 and b'repetition_penalty' in L.evk_last_error()
    assert beam(rp=-1.0) == -1 and b'repetition_penalty' in L.evk_last_error()
    assert beam(g=9) == -1 and b'no_repeat_ngram_size' in L.evk_last_error()
    assert beam(g=-1) == -1 and b'no_repeat_ngram_size' in L.evk_last_error()
    assert beam(ml=-1) == -1 and b'min_length' in L.evk_last_error()
    assert beam(nb=9) == -1 and b'nb must be' in L.evk_last_error()
    assert beam(nb=0) == -1
    assert beam(nb=4, V=7, ld=8) == -1 and b'candidates' in L.evk_last_error()
    assert beam(V=40, ld=39) == -1 and b'ld=' in L.evk_last_error()
    assert beam() == -1 and b'null' in L.evk_last_error()                   # (valid options and geometry, no buffers)
