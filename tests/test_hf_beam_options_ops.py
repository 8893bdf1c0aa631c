"""GPU tests of evk_hf_beam_step_opts (csrc/hf_beam.hip) through the C ABI against the step-by-step restatement
(tests/hf_beam_options_restatement.py): the whole search token by token at small geometry, single steps at late positions of the full
geometry, and the refusals.  tests/test_hf_beam_options_cpu.py asserts that the rows used here make every processor bite."""
import ctypes as C

import pytest
import torch

from tests import hf_beam_options_restatement as R
from tests.test_hf_beam_options_cpu import KERNEL_SETS, kernel_rows

pytestmark = pytest.mark.gpu


class _Dev:
    """the device arrays of one search, started from a restatement's state"""

    def __init__(self, ref, anc_cols):
        dev, B, nb, ml = 'cuda', ref.B, ref.nb, ref.max_len
        self.B, self.nb, self.ml, self.V, self.anc_cols = B, nb, ml, ref.V, anc_cols
        self.eos, self.pad = ref.eos, ref.pad
        self.seqs, self.scores, self.anc = ref.seqs.clone().to(dev), ref.scores.clone().to(dev), ref.anc.clone().to(dev)
        self.words = torch.full((B * nb,), -7, dtype=torch.long, device=dev)
        self.pos = torch.full((1,), ref.pos, dtype=torch.long, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hyp_score = torch.full((B, nb), -float('inf'), dtype=torch.float64, device=dev)
        self.hyp_len = torch.zeros(B, nb, dtype=torch.int32, device=dev)
        self.hyp_seq = torch.full((B, nb, ml), ref.pad, dtype=torch.long, device=dev)
        self.done = torch.tensor([int(d) for d in ref.done], dtype=torch.uint8, device=dev)
        self.n_done = torch.zeros(1, dtype=torch.int32, device=dev)
        o = ref.opts
        self.o = o
        self.len_div = None if o['length_penalty'] == 1.0 else torch.tensor(ref.div, dtype=torch.float64, device=dev)

    def step(self, logp, ld, last, **over):
        from evoke_amd import hip as H
        o = dict(self.o, **over)
        return H.lib.evk_hf_beam_step_opts(H.ptr(logp), ld, self.V, self.nb, self.B, self.ml, H.ptr(self.pos), self.eos, self.pad, int(last),
                                           H.ptr(self.scores), H.ptr(self.seqs), H.ptr(self.words), H.ptr(self.anc), self.anc_cols,
                                           H.ptr(self.hyp_score), H.ptr(self.hyp_len), H.ptr(self.hyp_seq), H.ptr(self.done), H.ptr(self.n_done),
                                           H.ptr(self.pos), H.ptr(self.ticket), C.c_float(o['repetition_penalty']), int(o['no_repeat_ngram_size']),
                                           int(o['min_length']), H.ptr(self.len_div) if self.len_div is not None else None,
                                           int(bool(o['early_stopping'])), H.stream())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _padded(rows, ld):
    logp = torch.full((rows.shape[0], ld), float('nan'), dtype=torch.float32)          # (a read or write beyond the V valid columns would show)
    logp[:, :rows.shape[1]] = rows
    return logp.cuda()


def _check_rows(logp, rows, ref, was_done, ld, what):
    """the processed rows of the studies that were live, as left in logp, bit for bit; a done study's rows and the pad columns untouched"""
    got, nb, V = logp.cpu(), ref.nb, ref.V
    assert bool(torch.isnan(got[:, V:]).all()), what
    for b in range(ref.B):
        sl = slice(b * nb, (b + 1) * nb)
        want = rows[sl] if was_done[b] else ref.rows[sl]
        assert torch.equal(_bits(got[sl, :V]), _bits(want)), (what, b)


@pytest.mark.parametrize('name', sorted(KERNEL_SETS))
@pytest.mark.parametrize('nb', [1, 2, 3, 4, 8])
@pytest.mark.parametrize('Vv,ld', [(37, 40), (1444, 1448)])
def test_hf_beam_step_opts_follows_the_restatement_step_by_step(Vv, ld, nb, name):
    from evoke_amd import hip as H
    B, max_len = 3, 12
    ref = R.HFBeamOpts(B, nb, Vv, max_len, Vv - 2, Vv - 1, 0, KERNEL_SETS[name], anc_cols=12)
    d = _Dev(ref, 12)
    for t in range(max_len - 1):
        rows = kernel_rows(Vv, nb, t)
        logp = _padded(rows, ld)
        last = t == max_len - 2
        was_done = list(ref.done)
        H.check(d.step(logp, ld, last), 'hf_beam_step_opts')
        ref.step(rows, force_end=last)
        what = '%s V=%d nb=%d step %d' % (name, Vv, nb, t)
        assert int(d.pos) == t + 1 == ref.pos, what
        assert torch.equal(d.words.cpu(), ref.words), what
        assert torch.equal(d.seqs.cpu(), ref.seqs), what
        assert torch.equal(d.anc.cpu(), ref.anc), what
        assert torch.equal(_bits(d.scores.cpu()), _bits(ref.scores)), what
        assert d.done.cpu().tolist() == [int(x) for x in ref.done], what
        assert int(d.n_done) == sum(ref.done) and int(d.ticket) == 0, what
        _check_rows(logp, rows, ref, was_done, ld, what)
    w_score, w_len, w_seq = ref.lists()
    assert torch.equal(d.hyp_len.cpu(), w_len) and bool((w_len > 0).all())
    assert torch.equal(d.hyp_seq.cpu(), w_seq)
    assert torch.equal(d.hyp_score.cpu(), w_score), (d.hyp_score.cpu(), w_score)          # f64, EQUAL: the host's divisor table


def test_neutral_options_write_the_bits_of_the_plain_step():
    """rp 1, g 0, min_length 0, no table, no early stopping: every array as evk_hf_beam_step leaves it, the rows untouched"""
    from evoke_amd import hip as H
    from tests.hf_beam_restatement import HFBeam
    B, nb, V, ld, max_len = 3, 3, 1444, 1448, 12
    ref = R.HFBeamOpts(B, nb, V, max_len, V - 2, V - 1, 0, None, anc_cols=12)
    a, b = _Dev(ref, 12), _Dev(ref, 12)
    for t in range(max_len - 1):
        rows = kernel_rows(V, nb, t)
        la, lb = _padded(rows, ld), _padded(rows, ld)
        last = t == max_len - 2
        H.check(a.step(la, ld, last), 'hf_beam_step_opts')
        H.check(H.lib.evk_hf_beam_step(H.ptr(lb), ld, V, nb, B, max_len, H.ptr(b.pos), V - 1, 0, int(last), H.ptr(b.scores), H.ptr(b.seqs),
                                       H.ptr(b.words), H.ptr(b.anc), 12, H.ptr(b.hyp_score), H.ptr(b.hyp_len), H.ptr(b.hyp_seq), H.ptr(b.done),
                                       H.ptr(b.n_done), H.ptr(b.pos), H.ptr(b.ticket), H.stream()), 'hf_beam_step')
        assert torch.equal(_bits(la), _bits(lb))
        for k in ('words', 'seqs', 'anc', 'done', 'n_done', 'pos', 'hyp_len', 'hyp_seq'):
            assert torch.equal(getattr(a, k), getattr(b, k)), (k, t)
        assert torch.equal(_bits(a.scores), _bits(b.scores)) and torch.equal(a.hyp_score.view(torch.int64), b.hyp_score.view(torch.int64)), t


@pytest.mark.parametrize('pos', [6, 7, 8, 250])
def test_late_positions_at_full_geometry(pos):
    """max_len 256, 8 beams, V 1444, 8-grams: one step at cur_len 7 (g - 1: no ban), 8 (the first ban), 9 and 251, on prefilled histories
    that repeat with period 3 (their 8-gram windows recur from cur_len 11 on) or hold one id throughout (the one window of cur_len 8 is a
    ban already); study 1 is done: its NaN rows stay untouched and it emits [PAD]"""
    from evoke_amd import hip as H
    B, nb, V, ld, max_len = 3, 8, 1444, 1448, 256
    opts = dict(repetition_penalty=1.3, no_repeat_ngram_size=8, min_length=252, length_penalty=0.7)
    ref = R.HFBeamOpts(B, nb, V, max_len, V - 2, V - 1, 0, opts, anc_cols=max_len)
    g = torch.Generator().manual_seed(41 + pos)
    hist = torch.randint(1, V - 2, (B * nb, 3), generator=g)
    for c in range(1, pos + 1):
        ref.seqs[:, c] = hist[:, c % 3]
    ref.seqs[::2, pos] = 5          # every other beam breaks the period at its last id: no window matches there
    ref.seqs[1::4] = ref.bos        # constant histories
    ref.pos = pos
    ref.scores = -torch.rand(B, nb, generator=g) * 3
    ref.anc = torch.randint(0, B * nb, (B * nb, max_len), generator=g, dtype=torch.int32)
    ref.done[1] = True
    d = _Dev(ref, max_len)
    rows = torch.log_softmax(torch.randn(B * nb, V, generator=g) * 2.0, -1)
    rows[:, ref.eos] += 6.0          # (an [EOS] that min_length has to keep out of the candidates)
    rows[nb:2 * nb] = float('nan')
    logp = _padded(rows, ld)
    was_done = list(ref.done)
    H.check(d.step(logp, ld, False), 'hf_beam_step_opts')
    live = [0, 2]
    after = ref_rows_after(ref, rows)
    assert bool(torch.isinf(after[:, ref.eos]).all())
    after[:, ref.eos] = 0.0
    banned = int(torch.isinf(after).sum())
    ref.step(rows)
    what = 'pos %d' % pos
    assert (banned > 0) == (pos + 1 >= 8) and (banned > 2 * 2) == (pos + 1 >= 11), (what, banned)          # (2 constant beams per live study)
    assert int(d.pos) == pos + 1
    assert torch.equal(d.words.cpu(), ref.words) and torch.equal(d.seqs.cpu(), ref.seqs) and torch.equal(d.anc.cpu(), ref.anc), what
    for b in live:
        assert torch.equal(_bits(d.scores.cpu()[b]), _bits(ref.scores[b])), what
    assert d.done.cpu().tolist() == [0, 1, 0] and int(d.n_done) == 0
    _check_rows(logp, rows, ref, was_done, ld, what)
    assert bool((d.words.cpu()[nb:2 * nb] == 0).all()) and bool((d.hyp_len.cpu() == 0).all())          # [EOS] is banned: no hypothesis yet


def ref_rows_after(ref, rows):
    """the live studies' rows as the processors leave them, without stepping the restatement"""
    out = R.process_rows(rows[:, :ref.V].float(), ref.seqs, ref.pos + 1, ref.nb, ref.done, ref.eos, ref.opts, ref.V)
    return torch.cat([out[:ref.nb], out[2 * ref.nb:]])


def test_hf_beam_step_opts_refuses_bad_arguments_before_any_launch():
    from evoke_amd import hip as H
    B, nb, V, ld, max_len = 3, 3, 37, 40, 12
    ref = R.HFBeamOpts(B, nb, V, max_len, V - 2, V - 1, 0, None, anc_cols=12)
    d = _Dev(ref, 12)
    rows = kernel_rows(V, nb, 0)
    logp = _padded(rows, ld)
    before = [t.clone() for t in (logp, d.seqs, d.scores, d.anc, d.pos, d.hyp_len, d.done, d.n_done)]
    for over, word in ((dict(repetition_penalty=0.0), b'repetition_penalty'), (dict(repetition_penalty=-1.5), b'repetition_penalty'),
                       (dict(no_repeat_ngram_size=9), b'no_repeat_ngram_size'), (dict(no_repeat_ngram_size=-1), b'no_repeat_ngram_size'),
                       (dict(min_length=-2), b'min_length')):
        assert d.step(logp, ld, False, **over) == -1 and word in H.lib.evk_last_error(), over
    assert d.step(logp, V - 1, False) == -1 and b'ld=' in H.lib.evk_last_error()
    d.nb = 9
    assert d.step(logp, ld, False) == -1 and b'nb must be' in H.lib.evk_last_error()
    d.nb = nb
    torch.cuda.synchronize()
    for was, now in zip(before, (logp, d.seqs, d.scores, d.anc, d.pos, d.hyp_len, d.done, d.n_done)):
        assert torch.equal(_bits(was) if was.dtype == torch.float32 else was, _bits(now) if now.dtype == torch.float32 else now)
