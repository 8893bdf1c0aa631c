"""CPU tests of the distilgpt2 backend's device-resident beam search: the restatement of the classic Hugging Face algorithm against a
recorded `generate` fixture, the coverage of the synthetic rows the GPU tests use, argument validation of the two new entry points,
and the interface errors of generate()."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.hf_beam_restatement import SCHEDULE, hf_beam_search, synthetic_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# what the GPU tests run (tests/test_hf_beam_gpu.py): (V, nb, max_len, seed) -- the kernel alone, then the whole session
KERNEL_SEED = {1: 2, 2: 29, 3: 2, 4: 2, 8: 2}          # nb = 2: the seed at which both vocabulary sizes reach the skip and the eviction
KERNEL_CASES = [(V, nb, 12, KERNEL_SEED[nb]) for V in (37, 1444) for nb in (1, 2, 3, 4, 8)]
SESSION_CASES = [(1444, nb, 12, seed) for nb in (3, 8) for seed in (2, 3)]
ALL_EARLY = ((1, 7.0), (1, 7.0), (2, 7.0))          # every study done within a few steps (the early-stop test)


def _pad_after_eos(seq, eos, pad, width):
    out = torch.full((seq.shape[0], width), pad, dtype=torch.long)
    out[:, :seq.shape[1]] = seq
    for r in range(out.shape[0]):
        hit = (out[r] == eos).nonzero()
        if len(hit):
            out[r, int(hit[0]) + 1:] = pad
    return out


def _fixture_cases():
    """-> dims, [(name, nb, n, max_length, [EOS] offset, weights, encoder states, logp_fn)] of tests/golden/hf_beam_tiny.npz"""
    from oracle import gpt2 as G
    gold = np.load(os.path.join(GOLDEN, 'hf_beam_tiny.npz'))
    dims = [int(v) for v in gold['dims']]
    V, D, layers, heads, B, S, bos, eos, pad = dims
    out = []
    for name in (str(c) for c in gold['cases']):
        seed, off, nb, n, ml = [int(tok.lstrip('sonbml_')) for tok in name.split('_')]
        P = {G.PRE + k[len('w%d/' % seed):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith('w%d/' % seed)}
        enc = torch.from_numpy(gold['enc%d' % seed])

        def logp_fn(step, rows, P=P, enc=enc, nb=nb, off=off):
            h, _ = G.gpt2_hidden(P, rows[:, :step + 1], None, enc.repeat_interleave(nb, 0), heads, layers)
            lg = h[:, -1] @ P[G.PRE + 'transformer.wte.weight'].t()
            lg[:, eos] += float(off)
            return torch.log_softmax(lg, -1)
        out.append((name, nb, n, ml, off, P, enc, logp_fn, torch.from_numpy(gold['case/%s/seq' % name]),
                    torch.from_numpy(gold['case/%s/score' % name])))
    return dims, out


def test_restatement_reproduces_the_recorded_hf_generate():
    """(a) sequences identical, scores within 1e-4 of transformers' generate for EVERY recorded case and every returned row
    (tests/golden/make_hf_beam_golden.py); everything after the first [EOS] of a row counts as [PAD] on both sides (the installed Hugging
    Face pads with [EOS]).

    The fixture was recorded with transformers 5.15, whose done test compares the list's worst entry with the best running beam; the classic
    scorer of the reference's pinned 4.23.1, which evk_hf_beam_step follows, compares it with the best candidate.  The restatement has a
    switch for that one line (done_test).  With 'running' all recorded cases are held in full: that validates candidates, rank walk,
    insertion, order, eviction and the force_end tail.  With 'candidate' the search is held (1) to the 'running' result, bit for bit, in
    every case where its own trace shows that the two tests never disagreed, and (2) to oracle.gpt2.beam_search, the restatement of the
    pinned release, on the best hypothesis of every case without an [EOS] offset (that function takes no offset)."""
    from oracle import gpt2 as G
    (V, D, layers, heads, B, S, bos, eos, pad), cases = _fixture_cases()
    assert len(cases) >= 60
    worst, agree = 0.0, []
    for name, nb, n, ml, off, P, enc, logp_fn, want, want_sc in cases:
        seqs, scores, _ = hf_beam_search(logp_fn, B, nb, V, ml, bos, eos, pad, n=n, done_test='running')
        assert seqs.shape[0] == want.shape[0] == B * n, name
        assert torch.equal(_pad_after_eos(seqs, eos, pad, ml), _pad_after_eos(want, eos, pad, ml)), name
        err = float((scores - want_sc).abs().max())
        worst = max(worst, err)
        assert err <= 1e-4, (name, err)
        c_seqs, c_scores, tr = hf_beam_search(logp_fn, B, nb, V, ml, bos, eos, pad, n=n, done_test='candidate')
        if sum(t['later_hf_differs'] for t in tr) == 0:
            agree.append(name)
            assert torch.equal(c_seqs, seqs) and torch.equal(c_scores, scores), name
        if off == 0:
            ref = G.beam_search(P, enc, heads, layers, nb, ml, bos, eos, pad)
            assert torch.equal(_pad_after_eos(c_seqs[::n], eos, pad, ml), _pad_after_eos(ref, eos, pad, ml)), name
    assert len(agree) >= 40
    for part in ('nb1_', 'nb2_', 'nb3_', 'nb4_', 'nb8_', '_n1_', '_n8_', 'ml6', 'ml12', '_o0_', '_o3_'):
        assert any(part in c for c in agree), part          # every axis of the case grid has cases where the releases agree throughout
    print('\n[hf beam fixture] %d cases in full, largest score difference %.2e; the two done tests agree throughout in %d' %
          (len(cases), worst, len(agree)))


def _trace(V, nb, max_len, seed, schedule=SCHEDULE, B=3):
    fn = lambda t, s: synthetic_rows(seed, t, B * nb, V, V - 1, nb, schedule)          # noqa: E731
    return hf_beam_search(fn, B, nb, V, max_len, V - 2, V - 1, 0, n=nb, stop_when_done=False)[2]


@pytest.mark.parametrize('V,nb,max_len,seed', sorted(set(KERNEL_CASES + SESSION_CASES)))
def test_synthetic_rows_reach_every_branch_of_the_search(V, nb, max_len, seed):
    """(b) so that a GPU pass cannot be vacuous: a study done strictly before the last step while another is not done at the end, a study
    closed by force_end, no ties among the candidates that matter, an [EOS] skipped at rank >= nb and an insertion into a full list that
    evicts an entry.  The last two cannot happen at nb = 1: the one source beam has one [EOS] candidate, which at rank >= 1 = nb is the
    second of two candidates and ends the walk unread, and the study is done on its first insertion.  The session cases of the GPU tests
    run at nb 3 and 8 only; the kernel cases cover nb = 2 (the kernel's narrow instantiation) with a seed of their own."""
    tr = _trace(V, nb, max_len, seed)
    assert len(tr) == max_len - 1
    assert any(any(t['done']) for t in tr[:-1]) and not all(tr[-1]['done'])
    assert sum(t['forced'] for t in tr) >= 1
    assert min(t['min_gap'] for t in tr) > 0
    if nb >= 2:
        assert sum(t['eos_skipped'] for t in tr) >= 1
        assert sum(t['evicted'] for t in tr) >= 1


def test_precondition_of_the_gpu_early_stop_test_every_study_is_done_early():
    """what test_search_stops_issuing_steps_once_every_study_is_done (GPU) relies on: beam 3, max_seq_len 64, seed 5, ALL_EARLY"""
    tr = _trace(1444, 3, 64, 5, ALL_EARLY)
    first = min(i for i, t in enumerate(tr) if all(t['done']))
    assert first <= 12, first


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    """(c) EINVAL before any HIP call"""
    from evoke_amd import hip as H
    L = H.lib

    def beam(nb=3, V=40, ld=40):
        return L.evk_hf_beam_step(None, ld, V, nb, 3, 12, None, V - 1, 0, 0, None, None, None, None, 12, None, None, None, None, None, None, None, None)
    assert beam(nb=9) == -1 and b'nb must be' in L.evk_last_error()
    assert beam(nb=0) == -1
    assert beam(nb=4, V=7, ld=8) == -1 and b'candidates' in L.evk_last_error()
    assert beam(V=40, ld=39) == -1 and b'ld=' in L.evk_last_error()
    assert beam() == -1 and b'null' in L.evk_last_error()                   # (valid geometry, no buffers)

    def attn(dh):
        return L.evk_decode_attention_wide(None, 0, None, None, None, None, None, None, None, None, 6, 24, 2, dh, 1, C.c_float(1.0), None)
    for dh in (64, 96):
        assert attn(dh) == -1 and b'head_dim must be 128 or 256' in L.evk_last_error()
    assert attn(128) == -1 and b'null' in L.evk_last_error()


def _decoder(**over):
    from evoke_amd.config import ARGS
    from evoke_amd.gpt2 import DistilGPT2TextDecoderModel
    from evoke_amd.tokenizer import load_tokenizer
    tok = load_tokenizer(os.path.join(GOLDEN, 'iu_xray_wordlevel_uncased_tokenizer.json'))
    args = dict(ARGS, decoder_hidden_size=64, decoder_num_hidden_layers=1, decoder_num_attention_heads=1, n_positions=32, max_seq_len=12, **over)
    return DistilGPT2TextDecoderModel(args, tok)


def test_generate_refuses_bad_beam_sizes_and_return_counts():
    """(d) before anything touches the device"""
    enc = torch.zeros(2, 5, 64)
    with pytest.raises(ValueError):
        _decoder(beam_size=9).generate(enc)
    with pytest.raises(ValueError):
        _decoder(beam_size=0).generate(enc)
    dec = _decoder(beam_size=3)
    for n in (0, 4):
        with pytest.raises(ValueError):
            dec.generate(enc, num_return_sequences=n)
    with pytest.raises(ValueError):
        _decoder(beam_size=3, sample_n=4).generate(enc)
