"""GPU tests of evk_decode_attention_maps (csrc/norm.hip) through the C ABI, against the float64 restatement tests/attn_maps_restatement.py
(its docstring derives the error bound from the operands).

Conventions: every output buffer is pre-filled with NaN and sits between guard bands that must come back untouched; the pad columns of the
map rows and the slabs the launch does not address must stay NaN; no index outside a buffer is ever passed.  Every case prints the worst
error it saw as a fraction of its bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import attn_maps_restatement as AR
from tests.helpers import STORE_DTYPE as BF

pytestmark = pytest.mark.gpu

F32 = torch.float32
G = 64                       # guard elements either side of an output
GUARD = 768.0               # exact in both 16-bit formats
EINVAL = -1
SCALE = 0.125


class Buf:
    """a device output of n elements, pre-filled with NaN, between two guard bands"""

    def __init__(self, n, dtype=F32):
        self.all = torch.full((n + 2 * G,), GUARD, dtype=dtype, device='cuda')
        self.t = self.all[G:G + n]
        self.t.fill_(float('nan'))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def cpu(self):
        g = self.all.cpu()
        assert bool((g[:G] == GUARD).all()) and bool((g[-G:] == GUARD).all()), 'a guard band was written'
        return g[G:-G]


# R, H, S, kv_div, mask
GEOMS = [
    (1, 1, 1, 1, 'none'),            # the map is exactly 1.0
    (3, 3, 5, 1, 'random'),          # 9 (row, head) pairs: idle waves in every workgroup; S < 8
    (8, 2, 50, 4, 'row1'),           # four query rows per K / V row; K / V row 1 fully masked: rows of zeros
    (6, 8, 81, 3, 'first80'),        # shared K / V rows, not a multiple of four; the running max still -inf after a whole 80-key batch
    (4, 8, 145, 1, 'none'),          # the token count of a 384 x 384 image with its global token
    (8, 8, 256, 4, 'random'),        # the maximum S
]


def operands(R, H, S, kv_div, mask_kind):
    """q, K of magnitude below 1 in the storage format: A = scale * max_s sum_i |q_i k_si| <= 0.125 * 64 = 8"""
    g = torch.Generator().manual_seed(7 + 1000 * R + S)
    Rk = R // kv_div
    q = (torch.rand(R, H * 64, generator=g) * 2 - 1).to(BF)
    k = (torch.rand(Rk, S, H * 64, generator=g) * 2 - 1).to(BF)
    v = (torch.rand(Rk, S, H * 64, generator=g) * 2 - 1).to(BF)
    # keys aligned with / opposed to row 0's query (same magnitudes, so A <= 8 holds): scores near +-4, weights spread over e^8
    sign = torch.sign(q[0].float()).to(BF)
    k[:, 1::5] = k[:, 1::5].abs() * sign
    k[:, 2::5] = -k[:, 2::5].abs() * sign
    mask = None
    if mask_kind == 'random':
        mask = (torch.rand(Rk, S, generator=g) < 0.6).to(torch.uint8)
        mask[:, S // 2] = 1
    elif mask_kind == 'row1':
        mask = torch.ones(Rk, S, dtype=torch.uint8)
        mask[1] = 0
    elif mask_kind == 'first80':
        mask = torch.ones(Rk, S, dtype=torch.uint8)
        mask[0, :80] = 0
    return q, k, v, mask


def launch(H_, q, k, v, mask, out, maps, ld, pos, stride, R, S, heads, kv_div, dh=64):
    return H_.lib.evk_decode_attention_maps(q.data_ptr(), k.data_ptr(), v.data_ptr(), mask.data_ptr() if mask is not None else None, out,
                                            maps, ld, pos.data_ptr() if pos is not None else None, stride, R, S, heads, dh, kv_div,
                                            C.c_float(SCALE), H_.stream())


@pytest.mark.parametrize('R,H,S,kv_div,mask_kind', GEOMS)
def test_attn_maps_kernel_against_the_float64_restatement(R, H, S, kv_div, mask_kind):
    from evoke_amd import hip as Hh
    q, k, v, mask = operands(R, H, S, kv_div, mask_kind)
    ref = AR.head_mean_softmax(q.double().view(R, H, 64).numpy(), k.double().view(R // kv_div, S, H, 64).numpy(),
                               None if mask is None else mask.numpy(), SCALE, kv_div)
    A = SCALE * np.einsum('rhd,rshd->rhs', np.abs(q.double().view(R, H, 64).numpy()),
                          np.abs(k.double().view(R // kv_div, S, H, 64).numpy())[np.arange(R) // kv_div]).max()
    assert A <= 8.0
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    md = mask.cuda() if mask is not None else None
    ld, n_slabs = S + 3, 4
    stride = R * ld + 5
    pos = torch.tensor([2], dtype=torch.long, device='cuda')
    # 1. the plain entry on the same inputs
    plain = Buf(R * H * 64, BF)
    Hh.check(Hh.lib.evk_decode_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), md.data_ptr() if md is not None else None, plain.ptr, R, S, H,
                                         64, kv_div, C.c_float(SCALE), Hh.stream()), 'decode_attention')
    runs = []
    for slab_pos in (pos, pos, None):
        out, maps = Buf(R * H * 64, BF), Buf(n_slabs * stride)
        Hh.check(launch(Hh, qd, kd, vd, md, out.ptr, maps.ptr, ld, slab_pos, stride, R, S, H, kv_div), 'decode_attention_maps')
        runs.append((out.cpu(), maps.cpu()))
    torch.cuda.synchronize()
    want_out = plain.cpu()
    assert not torch.isnan(want_out.float()).any()
    for out, _ in runs:
        assert torch.equal(out.view(torch.int16), want_out.view(torch.int16)), 'out differs from evk_decode_attention in its bits'
    # 2. only columns [0, S) of the R rows of the addressed slab are written
    written = torch.zeros(n_slabs * stride, dtype=torch.bool)
    for slab, (_, maps) in zip((2, 2, 0), runs):
        written.zero_()
        for r in range(R):
            written[slab * stride + r * ld: slab * stride + r * ld + S] = True
        assert torch.isnan(maps[~written]).all(), 'the launch wrote outside its rows (slab %d)' % slab
        assert not torch.isnan(maps[written]).any()
    got = torch.stack([runs[0][1][2 * stride + r * ld: 2 * stride + r * ld + S] for r in range(R)])
    got0 = torch.stack([runs[2][1][r * ld: r * ld + S] for r in range(R)])
    # 5. the same bits at every launch, wherever the slab
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)) and torch.equal(got.view(torch.int32), got0.view(torch.int32))
    g64 = got.double().numpy()
    keep = np.ones((R, S), dtype=bool) if mask is None else mask.numpy().astype(bool)[np.arange(R) // kv_div]
    assert (g64[~keep] == 0.0).all(), 'a masked key has a weight'
    assert (g64 >= 0).all()
    # 3. accuracy
    ratio = np.abs(g64 - ref['maps']) / ref['bound']
    rows = g64.sum(-1)
    alive = keep.any(-1)
    print('\n[attn maps R=%d H=%d S=%d kv_div=%d mask=%s] worst |map - float64| / bound = %.3f (A = %.2f); row sums within %.2e of 1 (allowed %.2e)'
          % (R, H, S, kv_div, mask_kind, ratio.max(), A, np.abs(rows[alive] - 1).max() if alive.any() else 0.0, (S + 2) * 2.0 ** -23))
    assert ratio.max() <= 1.0, 'beyond the bound at %s' % np.argwhere(ratio > 1)[:8].tolist()
    # 4. row sums
    assert (np.abs(rows[alive] - 1.0) <= (S + 2) * 2.0 ** -23).all()
    assert (rows[~alive] == 0).all()
    if S == 1:
        assert g64.tolist() == [[1.0]]


def test_attn_maps_entry_refuses_bad_arguments_and_writes_nothing():
    from evoke_amd import hip as Hh
    R, H, S = 4, 2, 9
    q, k, v, _ = operands(R, H, S, 1, 'none')
    qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
    out, maps = Buf(R * 256, BF), Buf(R * 300)
    bad = [dict(dh=128), dict(S=0), dict(S=257), dict(ld=S - 1), dict(R=3, kv_div=2), dict(maps=None)]
    for b in bad:
        a = dict(dict(dh=64, S=S, ld=300, R=R, kv_div=1, maps=maps.ptr), **b)
        st = launch(Hh, qd, kd, vd, None, out.ptr, a['maps'], a['ld'], None, 0, a['R'], a['S'], H, a['kv_div'], dh=a['dh'])
        assert st == EINVAL, (b, st)
        assert 'decode_attention_maps' in Hh.lib.evk_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out.cpu().float()).all() and torch.isnan(maps.cpu()).all()


def test_attn_maps_symbol_is_exported_by_both_libraries():
    import evoke_amd
    here = os.path.dirname(os.path.abspath(evoke_amd.__file__))
    for name in ('libevoke_hip.so', 'libevoke_hip_bf16.so'):
        lib = C.CDLL(os.path.join(here, name))
        assert hasattr(lib, 'evk_decode_attention_maps'), name
