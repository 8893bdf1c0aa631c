"""CPU tests of the distilgpt2 backend's sampling route: the restatement of Hugging Face's logits processors and choice
(tests/hf_sample_restatement.py) against what the installed `generate` recorded (tests/golden/hf_sample_tiny.npz, written by
tests/golden/make_hf_sample_golden.py), its inverse-CDF draw against the kept entries' probabilities, the argument checks of
DistilGPT2TextDecoderModel.generate that need no GPU, and the library's export of evk_hf_sample_step."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import hf_sample_restatement as HS
from tests.helpers import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT_KEYS = tuple(HS.NEUTRAL)


@pytest.fixture(scope='module')
def fixture():
    z = np.load(os.path.join(GOLDEN, 'hf_sample_tiny.npz'))
    V, B, bos, eos, pad = [int(v) for v in z['dims']]
    return z, json.loads(str(z['options'])), dict(V=V, B=B, bos=bos, eos=eos, pad=pad)


def test_hf_sample_fixture_covers_the_case_grid(fixture):
    z, options, _ = fixture
    cases = [str(c) for c in z['cases']]
    assert len(cases) == len(set(cases)) == len(options)
    sets = {tuple(sorted((k, o[k]) for k in OPT_KEYS)) for o in options.values()}
    want = [dict(do_sample=True), dict(do_sample=True, temperature=0.7, top_k=5),
            dict(do_sample=True, temperature=1.3, top_p=0.8, no_repeat_ngram_size=2, min_length=4),
            dict(do_sample=True, repetition_penalty=1.2, no_repeat_ngram_size=3, top_k=10, top_p=0.9), dict(do_sample=True, top_k=1),
            dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(min_length=6),
            dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_length=6)]
    for w in want:
        key = tuple(sorted(HS.options(**w).items()))
        assert key in sets, w
        mine = [o for o in options.values() if tuple(sorted((k, o[k]) for k in OPT_KEYS)) == key]
        assert {o['max_length'] for o in mine} == {6, 12} and {o['eos_offset'] for o in mine} == {0.0, 3.0}
        assert {o['n'] for o in mine} == ({1, 3} if w.get('do_sample') else {1})
    kept = sum(int(z['case/%s/keep' % c].sum()) for c in cases)
    rows = sum(z['case/%s/keep' % c].size for c in cases)
    assert kept >= 0.95 * rows, (kept, rows)


def test_restatement_reproduces_the_recorded_processed_scores(fixture):
    """teacher-forced on the recorded ids, fed the recorded raw logits: for every kept row the same finite set exactly and the finite values
    to 1e-5; greedy cases reproduce the recorded ids; rows after [EOS] are [PAD]; the copies of a study are neighbours"""
    z, options, d = fixture
    eos, pad, bos, B = d['eos'], d['pad'], d['bos'], d['B']
    worst, n_rows = 0.0, 0
    for name, o in options.items():
        opts = {k: o[k] for k in OPT_KEYS}
        seq = torch.from_numpy(z['case/%s/seq' % name])
        scores, logits, keep = torch.from_numpy(z['case/%s/scores' % name]), torch.from_numpy(z['case/%s/logits' % name]), z['case/%s/keep' % name]
        R, L = seq.shape
        assert R == B * o['n'] and L <= o['max_length'] and bool((seq[:, 0] == bos).all()), name
        assert scores.shape[0] == L - 1
        for r in range(R):
            ids = seq[r].tolist()
            if eos in ids:
                assert all(i == pad for i in ids[ids.index(eos) + 1:]), (name, r)
        alive = torch.ones(R, dtype=torch.bool)
        for t in range(L - 1):
            for r in range(R):
                pr = HS.process_row(logits[t, r], seq[r, :t + 1].tolist(), eos, opts)
                if not keep[t, r]:
                    continue
                want, got = scores[t, r], pr['row']
                fin = torch.isfinite(want)
                assert torch.equal(torch.isfinite(got), fin), (name, t, r)
                assert bool((got[~fin] == want[~fin]).all())
                worst = max(worst, float((got[fin] - want[fin]).abs().max()))
                n_rows += 1
                if alive[r]:
                    # the recorded id is one the processed row allows; the greedy id is the restatement's own
                    assert bool(torch.isfinite(got[seq[r, t + 1]])), (name, t, r)
                    if not opts['do_sample']:
                        assert HS.choose(got, False, None, pad)[0] == int(seq[r, t + 1]), (name, t, r)
                else:
                    assert int(seq[r, t + 1]) == pad
            alive &= seq[:, t + 1] != eos
        if o['n'] == 3 and opts['top_k'] == 1:
            # top_k 1 leaves one entry: the three copies of a study draw the same ids, and they sit next to each other
            assert torch.equal(seq[0::3], seq[1::3]) and torch.equal(seq[0::3], seq[2::3]), name
        if o['n'] == 3:
            # the copies of a study read the study's encoder rows: their raw logits of the first step are the same rows
            assert torch.equal(logits[0, 0::3], logits[0, 1::3]) and torch.equal(logits[0, 0::3], logits[0, 2::3]), name
            assert not torch.equal(logits[0, 0], logits[0, 3])
    print('\n[hf sample fixture] %d rows, largest difference of a finite processed score %.3e' % (n_rows, worst))
    assert n_rows > 2000 and worst <= 1e-5, worst


def test_token_loop_of_the_restatement_reproduces_the_greedy_cases(fixture):
    """the whole loop (step / generate) fed the recorded raw logits of the greedy cases: the recorded ids, lengths and finished rows"""
    z, options, d = fixture
    for name, o in options.items():
        if o['do_sample'] or not z['case/%s/keep' % name].all():
            continue
        opts = {k: o[k] for k in OPT_KEYS}
        seq, logits = torch.from_numpy(z['case/%s/seq' % name]), torch.from_numpy(z['case/%s/logits' % name])
        R, L = seq.shape
        got = HS.generate(lambda t, s: logits[t], R, L, d['bos'], d['eos'], d['pad'], opts)
        assert torch.equal(got['seqs'], seq), name
        for r in range(R):
            ids = seq[r].tolist()
            assert int(got['lengths'][r]) == (ids.index(d['eos']) + 1 if d['eos'] in ids else L)
        assert bool((got['tok_logp'][:, 0] == 0).all()) and bool((got['tok_logp'] <= 0).all())


def test_inverse_cdf_draw_follows_the_kept_probabilities():
    """20 000 uniforms on one fixed row: every kept entry's frequency within 4 standard errors of its probability, no removed entry drawn"""
    g = torch.Generator().manual_seed(3)
    row = torch.randn(60, generator=g) * 2.0
    hist = [58, 7, 9, 7]
    opts = HS.options(do_sample=True, temperature=0.9, top_k=12, top_p=0.95, repetition_penalty=1.1, no_repeat_ngram_size=2)
    pr = HS.process_row(row, hist, 59, opts)['row']
    w = HS.weights(pr)
    prob = w / w.sum()
    kept = np.nonzero(w > 0)[0]
    assert 3 <= len(kept) <= 12 and not np.isfinite(float(pr[9]))            # (7, 9) was seen: 9 is banned after 7
    N = 20000
    us = torch.rand(N, generator=g, dtype=torch.float64).numpy()
    counts = np.zeros(60)
    for u in us:
        counts[HS.draw(w, u)[0]] += 1
    assert counts[w == 0].sum() == 0
    for i in kept:
        se = np.sqrt(prob[i] * (1 - prob[i]) / N)
        assert abs(counts[i] / N - prob[i]) <= 4 * se, (i, counts[i] / N, prob[i], se)
    assert HS.draw(w, 0.0)[0] == kept[0] and HS.draw(w, 1.0 - 1e-12)[0] == kept[-1]


def test_processors_one_by_one_on_hand_made_rows():
    x = torch.tensor([2.0, -1.0, 0.5, 3.0, -2.0, 1.0])
    r = HS.process_row(x, [5, 1, 1], 4, HS.options(repetition_penalty=2.0))['row']
    assert r.tolist() == [2.0, -2.0, 0.5, 3.0, -2.0, 0.5]                      # distinct ids once; the sign decides
    assert HS.banned_ngram_ids([5, 1, 2, 1], 2) == [2] and HS.banned_ngram_ids([5, 1], 3) == [] and HS.banned_ngram_ids([5, 1, 1], 1) == [1, 5]
    assert HS.banned_ngram_ids([5, 1, 2, 3, 1, 2], 3) == [3]
    r = HS.process_row(x, [5], 3, HS.options(min_length=2))['row']
    assert r[3] == float('-inf') and HS.choose(r, False, None, 0)[0] == 0
    r = HS.process_row(x, [5, 0], 3, HS.options(min_length=2))['row']
    assert HS.choose(r, False, None, 0)[0] == 3
    tie = torch.tensor([1.0, 3.0, 2.0, 2.0, 0.0])
    r = HS.process_row(tie, [4], 0, HS.options(do_sample=True, top_k=2))['row']
    assert torch.isfinite(r).tolist() == [False, True, True, True, False]      # both entries at the k-th value stay
    r = HS.process_row(tie, [4], 0, HS.options(do_sample=True, top_p=1e-6))['row']
    assert torch.isfinite(r).tolist() == [False, True, False, False, False]    # the maximum always stays
    none = torch.full((5,), float('-inf'))
    assert HS.choose(none, True, 0.3, 2) == (2, 0.0, np.inf)


class _Tok:
    def token_to_id(self, t):
        return {'[PAD]': 0, '[BOS]': 38, '[EOS]': 39}[t]


def _tiny(**cfg):
    from evoke_amd.gpt2 import DistilGPT2TextDecoderModel
    return DistilGPT2TextDecoderModel(dict(dict(decoder_hidden_size=64, vocab_size=40, decoder_num_attention_heads=1, decoder_num_hidden_layers=1,
                                                beam_size=1, max_seq_len=8, n_positions=16), **cfg), _Tok())


def test_generate_checks_the_new_keywords_before_it_touches_the_device():
    dec = _tiny()
    enc = torch.zeros(2, 3, 64)
    for kw, word in ((dict(do_sample=True, temperature=0.0), 'temperature'), (dict(do_sample=True, temperature=-1.5), '-1.5'),
                     (dict(do_sample=True, top_p=0.0), 'top_p'), (dict(do_sample=True, top_p=1.5), '1.5'), (dict(do_sample=True, top_k=-3), '-3'),
                     (dict(repetition_penalty=0.0), 'repetition_penalty'), (dict(repetition_penalty=-2.0), '-2.0'),
                     (dict(no_repeat_ngram_size=9), '9'), (dict(repetition_penalty=1.2, num_return_sequences=2), 'num_return_sequences'),
                     (dict(do_sample=True, uniforms=torch.zeros(2, 7)), 'uniforms'),
                     (dict(do_sample=True, uniforms=torch.zeros(2, 8, dtype=torch.float64)), 'uniforms'),
                     (dict(do_sample=True, num_return_sequences=3, uniforms=torch.zeros(2, 8)), 'uniforms')):
        with pytest.raises(ValueError, match=re.escape(word)):
            dec.generate(enc, **kw)
    dec3 = _tiny(beam_size=3)
    with pytest.raises(NotImplementedError, match='beam_size 1'):
        dec3.generate(enc, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match='beam_size 1'):
        _tiny(beam_size=3, do_sample=True, top_k=5).generate(enc)
    # the configuration's keys are the defaults; None and the neutral values leave the beam search as it is
    assert dec._generation_options(None, None, None, None, None, None, None) is None
    assert dec._generation_options(False, 1.0, 0, 1.0, 1.0, 0, 0) is None
    assert dec._generation_options(None, 0.7, 5, 0.9, None, None, None) is None          # warpers without do_sample: inert, as in HF
    o = _tiny(do_sample=True, top_k=5, temperature=0.7)._generation_options(None, None, None, None, 1.2, None, None)
    assert o == dict(do_sample=True, temperature=0.7, top_k=5, top_p=1.0, repetition_penalty=1.2, no_repeat_ngram_size=0, min_length=0)
    assert _tiny(do_sample=True)._generation_options(False, None, None, None, None, None, None) is None


def test_library_exports_the_hf_sample_step():
    from evoke_amd import build
    path = build.build()
    txt = open(os.path.join(REPO, 'include', 'evoke_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+evk_hf_sample_step\s*\(', txt)
    for lib_path in (path, build.LIB_BF16):
        assert hasattr(ctypes.CDLL(lib_path), 'evk_hf_sample_step'), lib_path
