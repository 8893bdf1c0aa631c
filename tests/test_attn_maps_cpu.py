"""CPU tests of the attention-map feature: the fixture's own properties (tests/golden/make_attn_maps_golden.py), decode.attention_grid, the
float64 restatement tests/attn_maps_restatement.py against torch, and the host-side validation of return_attention.  The fixture stores the
maps and the encoder states, not the reference's q / K, so the restatement is pinned to torch's softmax on synthetic 16-bit operands."""
import os

import numpy as np
import pytest
import torch

from tests import attn_maps_restatement as AR
from tests.golden.cases import CASES
from tests.helpers import GOLDEN, V

BASE = 'beam224_b4'


def load():
    return np.load(os.path.join(GOLDEN, BASE + '_attn.npz'))


def test_attn_maps_fixture_shapes_and_row_sums():
    g, case = load(), CASES[BASE]
    B, S, d = g['enc'].shape
    assert (B, d) == (case['B'], 512) and S == (case['res'] // 32) ** 2          # the decoder attends to the patches: no global token
    assert g['enc'].dtype == np.float32
    assert g['beam/ids'].tolist() == np.load(os.path.join(GOLDEN, BASE + '.npz'))['eval/seq'].tolist()
    assert g['greedy/ids'].tolist() == np.load(os.path.join(GOLDEN, 'sample224_greedy.npz'))['seq'].tolist()
    for name in ('beam', 'greedy'):
        ids, maps, drift = g[name + '/ids'], g[name + '/maps'], g[name + '/drift16']
        L = ids.shape[1]
        assert maps.shape == drift.shape == (B, L, 3, S) and maps.dtype == drift.dtype == np.float32
        assert not (ids == V - 1).any() and not (ids == 0).any()                  # no [EOS], no [PAD]: every position is a word
        assert (maps >= 0).all() and (drift >= 0).all()
        assert np.abs(maps.astype(np.float64).sum(-1) - 1.0).max() <= 1e-6
        assert 0 < drift.max() < 1e-2 * maps.max()                                # the 16-bit drift is a small fraction of a weight
    assert os.path.getsize(os.path.join(GOLDEN, BASE + '_attn.npz')) < os.path.getsize(os.path.join(GOLDEN, 'hf_sample_tiny.npz'))


def test_attn_maps_attention_grid_shapes_values_and_refusal():
    from evoke_amd import decode
    att = torch.arange(2 * 3 * 2 * 13, dtype=torch.float32).view(2, 3, 2, 13)
    glob, patches = decode.attention_grid(att, (3, 4))
    assert tuple(glob.shape) == (2, 3, 2) and tuple(patches.shape) == (2, 3, 2, 3, 4)
    assert torch.equal(glob, att[..., 0])
    for i in range(3):
        for j in range(4):
            assert torch.equal(patches[..., i, j], att[..., 1 + 4 * i + j])       # row-major behind the global token
    glob1, patches1 = decode.attention_grid(att[0, 0, 0], (4, 3))
    assert tuple(glob1.shape) == () and tuple(patches1.shape) == (4, 3) and patches1[1, 0].item() == att[0, 0, 0, 4].item()
    g2, p2 = decode.attention_grid(att.numpy(), (3, 4))                           # arrays as well as tensors
    assert g2.shape == (2, 3, 2) and p2.shape == (2, 3, 2, 3, 4)
    for bad in ((3, 3), (13, 1), (4, 4), (0, 12), (12, 0), (-3, -4)):
        with pytest.raises(ValueError):
            decode.attention_grid(att, bad)
    with pytest.raises(ValueError):
        decode.attention_grid(torch.ones(2, 1), (1, 1))


@pytest.mark.parametrize('R,H,S,kv_div,mask_kind', [(1, 1, 1, 1, 'none'), (3, 3, 5, 1, 'random'), (8, 2, 50, 4, 'row1'), (6, 8, 81, 3, 'first80')])
def test_attn_maps_restatement_equals_torch_softmax(R, H, S, kv_div, mask_kind):
    """the float64 restatement on 16-bit operands against torch's own masked softmax in float64, and the properties its bound relies on"""
    g = torch.Generator().manual_seed(R * 1000 + S)
    q = torch.randn(R, H, 64, generator=g).half()
    k = torch.randn(R // kv_div, S, H, 64, generator=g).half()
    mask = None
    if mask_kind == 'random':
        mask = (torch.rand(R // kv_div, S, generator=g) < 0.6).to(torch.uint8)
        mask[:, 0] = 1
    elif mask_kind == 'row1':
        mask = torch.ones(R // kv_div, S, dtype=torch.uint8)
        mask[1] = 0
    elif mask_kind == 'first80':
        mask = torch.ones(R // kv_div, S, dtype=torch.uint8)
        mask[0, :80] = 0
    res = AR.head_mean_softmax(q.numpy(), k.numpy(), None if mask is None else mask.numpy(), 0.125, kv_div)
    kk = k.double().repeat_interleave(kv_div, 0)
    x = 0.125 * torch.einsum('rhd,rshd->rhs', q.double(), kk)
    if mask is not None:
        keep = mask.bool().repeat_interleave(kv_div, 0).unsqueeze(1)
        x = x.masked_fill(~keep, -float('inf'))
    p = torch.softmax(x, -1)
    p = torch.where(torch.isnan(p), torch.zeros_like(p), p)                       # a row without keys: zeros
    want = p.mean(1).numpy()
    assert res['maps'].shape == (R, S) and np.abs(res['maps'] - want).max() <= 1e-15
    if mask is not None:
        dead = ~mask.bool().repeat_interleave(kv_div, 0).numpy()
        assert (res['maps'][dead] == 0).all()
        if mask_kind == 'row1':
            assert (res['maps'][4:8] == 0).all() and (res['bound'][4:8] == AR.FLOOR).all()
    rows = res['maps'].sum(-1)
    assert np.all((np.abs(rows - 1) < 1e-12) | (rows == 0))
    assert (res['bound'] >= AR.FLOOR).all() and (res['bound'] <= res['maps'] * AR.U * (128 * 64 + 400) + AR.FLOOR).all()
    if S == 1:
        assert res['maps'].tolist() == [[1.0]]


def test_attn_maps_option_validation_without_the_library_doing_work():
    """return_attention joins the beam options only when set (the session keys of every other search stay what they were); bad options are
    still refused first"""
    from evoke_amd import decode
    base = dict(beam_size=4, max_seq_len=14)
    assert decode.beam_options(base, 4) is None
    assert decode.beam_options(base, 4, return_attention=False) is None
    opts = decode.beam_options(base, 4, return_attention=True)
    assert opts == dict(temperature=1.0, decoding_constraint=0, length_penalty='', sample_n=1, return_logprobs=False, return_attention=True)
    assert 'return_attention' not in decode.beam_options(base, 4, return_logprobs=True)
    assert decode.beam_options(dict(base, sample_n=4), 4, return_logprobs=True, return_attention=True)['return_attention'] is True
    with pytest.raises(ValueError):
        decode.beam_search(None, None, None, dict(base, sample_n=3), return_attention=True)
    with pytest.raises(NotImplementedError):
        decode.beam_search(None, None, None, dict(base, group_size=2), return_attention=True)
    import inspect
    assert inspect.signature(decode.beam_search).parameters['return_attention'].default is False
    assert inspect.signature(decode.sample).parameters['return_attention'].default is False
    from evoke_amd.model_pretrain_finetune import FineTune
    assert list(inspect.signature(FineTune.generate_with_attention).parameters) == ['self', 'images', 'patient_ids', 'inc_ids', 'inc_masks']
