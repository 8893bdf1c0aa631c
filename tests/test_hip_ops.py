"""GPU unit parity of the row-wise / BN / elementwise kernels and the autograd wrappers (evoke_amd.ops, trunk,
losses) against plain torch fp32 references evaluated on the same bf16-rounded inputs."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
from tests.helpers import STORE_DTYPE as BF      # bf16, or fp16 under EVK_STORE=f16
from tests.helpers import F16_BUILD, NO_F16_GRADS


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, want, rtol, atol, what=''):
    got, want = got.detach().float().cpu(), want.detach().float()
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    assert bool((err <= tol).all()), '%s max err %.4g (tol %.4g), rel-norm %.3g' % (
        what, err.max().item(), tol.flatten()[err.argmax()].item(), (err.norm() / (want.norm() + 1e-30)).item())


def leaf(t, dtype=BF):
    return t.to(dtype).cuda().requires_grad_(True)


def ref(t):
    return t.to(BF).float().requires_grad_(True)


@pytest.mark.parametrize('mode,D', [(0, 2048), (0, 768), (1, 512)])
def test_layernorm(mode, D):
    from evoke_amd import ops
    x, g, b = rnd(37, D, seed=1), 1 + 0.2 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dy = rnd(37, D, seed=4)
    xd, gd, bd = leaf(x), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    eps = 1e-5 if mode == 0 else 1e-6
    y = ops.layernorm(xd, gd, bd, eps=eps, mode=mode)
    y.backward(dy.to(BF).cuda())
    xr, gr, br = ref(x), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    if mode == 0:
        yr = F.layer_norm(xr, (D,), gr, br, eps)
    else:
        yr = gr * (xr - xr.mean(-1, keepdim=True)) / (xr.std(-1, keepdim=True) + eps) + br
    yr.backward(dy.to(BF).float())
    close(y, yr, 1e-2, 1e-2, 'y')
    close(xd.grad, xr.grad, 2e-2, 2e-2, 'dx')
    close(gd.grad, gr.grad, 1e-2, 5e-2, 'dgamma')
    close(bd.grad, br.grad, 1e-2, 5e-2, 'dbeta')


def test_conditional_layernorm():
    from evoke_amd import ops
    D, R = 512, 45
    x, g, b = rnd(R, D, seed=1), 1 + 0.2 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dg_, db_ = 0.3 * rnd(R, D, seed=5), 0.3 * rnd(R, D, seed=6)
    dy = rnd(R, D, seed=4)
    xd, gd, bd, dgd, dbd = leaf(x), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True), leaf(dg_), leaf(db_)
    y = ops.layernorm(xd, gd, bd, eps=1e-6, mode=1, dgam=dgd, dbet=dbd)
    y.backward(dy.to(BF).cuda())
    xr, gr, br, dgr, dbr = ref(x), g.clone().requires_grad_(True), b.clone().requires_grad_(True), ref(dg_), ref(db_)
    yr = (gr + dgr) * (xr - xr.mean(-1, keepdim=True)) / (xr.std(-1, keepdim=True) + 1e-6) + (br + dbr)
    yr.backward(dy.to(BF).float())
    close(y, yr, 1e-2, 1e-2, 'y')
    close(xd.grad, xr.grad, 2e-2, 2e-2, 'dx')
    close(dgd.grad, dgr.grad, 1e-2, 1e-2, 'ddgam')
    close(dbd.grad, dbr.grad, 1e-2, 1e-2, 'ddbet')
    close(gd.grad, gr.grad, 1e-2, 5e-2, 'dgamma')


@pytest.mark.parametrize('act', ['none', 'relu'])
def test_linear_fwd_bwd(act):
    from evoke_amd import hip as H, ops
    M, K, N = 290, 512, 1445
    x, W, b = rnd(2, M // 2, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), 0.1 * rnd(N, seed=3)
    xd, Wd, bd = leaf(x), W.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = ops.linear(xd, Wd, bd, act=H.ACT_RELU if act == 'relu' else H.ACT_NONE, out_f32=(act == 'none'))
    assert y.shape[-1] == 1448 and float(y[..., N:].abs().sum()) == 0
    dy = rnd(2, M // 2, 1448, seed=4)
    dy[..., N:] = 0
    y.backward(dy.to(y.dtype).cuda())
    xr, Wr, br = ref(x), W.to(BF).float().requires_grad_(True), b.clone().requires_grad_(True)
    yr = F.linear(xr, Wr, br)
    if act == 'relu':
        yr = F.relu(yr)
    yr.backward(dy[..., :N].to(BF).float())
    close(y[..., :N], yr, 1e-2, 1e-2, 'y')
    close(xd.grad, xr.grad, 2e-2, 3e-2, 'dx')
    close(Wd.grad, Wr.grad, 2e-2, 5e-2, 'dW')
    close(bd.grad, br.grad, 2e-2, 5e-2, 'db')


@pytest.mark.parametrize('cfg', [dict(B=3, T=37, S=50, Hh=12, dh=64, mask='key'), dict(B=2, T=20, S=20, Hh=8, dh=64, mask='causal'),
                                 dict(B=2, T=145, S=290, Hh=8, dh=256, mask=None), dict(B=4, T=3, S=4, Hh=8, dh=64, mask=None),
                                 dict(B=2, T=145, S=435, Hh=8, dh=2048, mask=None),          # multi-view fusion: 3 siblings, 2048-wide heads
                                 dict(B=2, T=100, S=100, Hh=8, dh=64, mask='causal'),        # decoder self-attention at max_seq_len
                                 dict(B=3, T=33, S=70, Hh=4, dh=64, mask='full')])           # per-query mask [B, T, S]
def test_attention(cfg):
    from evoke_amd import ops
    B, T, S, Hh, dh = cfg['B'], cfg['T'], cfg['S'], cfg['Hh'], cfg['dh']
    q, k, v = rnd(B, T, Hh * dh, seed=1), rnd(B, S, Hh * dh, seed=2), rnd(B, S, Hh * dh, seed=3)
    do = rnd(B, T, Hh * dh, seed=4)
    mask = None
    if cfg['mask'] == 'full':
        mask = (torch.rand(B, T, S, generator=torch.Generator().manual_seed(9)) > 0.3).to(torch.uint8)
        mask[:, :, 0] = 1
    elif cfg['mask']:
        mask = torch.ones(B, S, dtype=torch.uint8)
        for i in range(B):
            mask[i, S - 3 * i:] = 0
    qd, kd, vd = leaf(q), leaf(k), leaf(v)
    o = ops.attention(qd, kd, vd, Hh, mask=mask.cuda() if mask is not None else None, causal=cfg['mask'] == 'causal')
    o.backward(do.to(BF).cuda())
    qr, kr, vr = ref(q), ref(k), ref(v)
    sc = torch.einsum('bthd,bshd->bhts', qr.view(B, T, Hh, dh), kr.view(B, S, Hh, dh)) / math.sqrt(dh)
    if mask is not None:
        sc = sc.masked_fill((mask[:, None, :, :] if mask.dim() == 3 else mask[:, None, None, :]) == 0, -1e9)
    if cfg['mask'] == 'causal':
        sc = sc.masked_fill(torch.tril(torch.ones(T, S)) == 0, -1e9)
    orf = torch.einsum('bhts,bshd->bthd', torch.softmax(sc, -1), vr.view(B, S, Hh, dh)).reshape(B, T, Hh * dh)
    orf.backward(do.to(BF).float())
    close(o, orf, 2e-2, 2e-2, 'o')
    close(qd.grad, qr.grad, 3e-2, 3e-2, 'dq')
    close(kd.grad, kr.grad, 3e-2, 3e-2, 'dk')
    close(vd.grad, vr.grad, 3e-2, 3e-2, 'dv')


def test_fused_attention_dropout_through_the_c_abi():
    """evk_attention_fwd / evk_attention_bwd (csrc/attn.hip) called directly with attention dropout 0.1: the post-dropout
    probabilities the kernel writes define the keep mask; output, dQ and dS are then checked against the f32 formulas with THAT
    mask, and the same seed must reproduce the same mask in the backward (stateless hash + seed epoch)."""
    import ctypes as C
    from evoke_amd import hip as H
    B, T, S, Hh, dh, p = 2, 45, 77, 4, 64, 0.1
    Sp = (S + 7) // 8 * 8
    q, k, v, do = (rnd(B, n, Hh * dh, seed=i).to(BF).cuda() for i, n in ((1, T), (2, S), (3, S), (4, T)))
    out, dq = torch.empty_like(q), torch.empty_like(q)
    P, Pd, dS = (torch.zeros(B, Hh, T, Sp, dtype=BF, device='cuda') for _ in range(3))
    scale, seed = 1.0 / math.sqrt(dh), 1234567
    H.check(H.lib.evk_attention_fwd(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(out), H.ptr(P), H.ptr(Pd), None, 0, 0, 0, B, Hh, T, S, dh,
                                    C.c_float(scale), C.c_float(p), C.c_uint64(seed), H.stream()))
    H.check(H.lib.evk_attention_bwd(H.ptr(do), H.ptr(k), H.ptr(v), H.ptr(P), H.ptr(dS), H.ptr(dq), B, Hh, T, S, dh, C.c_float(scale),
                                    C.c_float(p), C.c_uint64(seed), H.stream()))
    qf, kf, vf, dof = (t.float().cpu().view(B, -1, Hh, dh) for t in (q, k, v, do))
    Pf, Pdf = P.float().cpu()[..., :S], Pd.float().cpu()[..., :S]
    pr = torch.softmax(torch.einsum('bthd,bshd->bhts', qf, kf) * scale, -1)
    keep = (Pdf != 0).float()
    frac = float(keep.mean())
    assert abs(frac - (1 - p)) < 0.02, frac
    close(Pf, pr, 1e-2, 1e-3, 'P')
    close(Pdf, pr * keep / (1 - p), 1e-2, 1e-3, 'P dropped')
    close(out.view(B, T, Hh, dh), torch.einsum('bhts,bshd->bthd', Pdf, vf), 1e-2, 1e-2, 'out')
    dP = torch.einsum('bthd,bshd->bhts', dof, vf) * keep / (1 - p)
    dSr = Pf * (dP - (dP * Pf).sum(-1, keepdim=True)) * scale
    close(dS.float().cpu()[..., :S], dSr, 2e-2, 2e-3, 'dS')
    close(dq.view(B, T, Hh, dh), torch.einsum('bhts,bshd->bthd', dS.float().cpu()[..., :S], kf), 1e-2, 1e-2, 'dQ')


@pytest.mark.parametrize('C_,relu,res', [(64, True, False), (256, True, True), (2048, False, False)])
def test_batchnorm_train(C_, relu, res):
    from evoke_amd.trunk import BNP
    M = 600
    x, r = rnd(M, C_, seed=1, scale=2.0) + 0.5, rnd(M, C_, seed=2)
    dz = rnd(M, C_, seed=3)
    bn = BNP(C_).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * rnd(C_, seed=4))
        bn.bias.copy_(0.1 * rnd(C_, seed=5))
    xd = leaf(x)
    rd = leaf(r) if res else None
    z = bn(xd, relu=relu, resid=rd)
    z.backward(dz.to(BF).cuda())
    tb = torch.nn.BatchNorm1d(C_).train()
    with torch.no_grad():
        tb.weight.copy_(bn.weight.cpu())
        tb.bias.copy_(bn.bias.cpu())
    xr = ref(x)
    rr = ref(r) if res else None
    zr = tb(xr)
    if res:
        zr = zr + rr
    if relu:
        zr = F.relu(zr)
    zr.backward(dz.to(BF).float())
    close(z, zr, 2e-2, 2e-2, 'z')
    close(xd.grad, xr.grad, 3e-2, 3e-2, 'dx')
    if res:
        close(rd.grad, rr.grad, 1e-2, 1e-2, 'dres')
    close(bn.weight.grad, tb.weight.grad, 2e-2, 0.3, 'dgamma')
    close(bn.bias.grad, tb.bias.grad, 2e-2, 0.3, 'dbeta')
    close(bn.running_mean, tb.running_mean, 1e-2, 1e-3, 'running_mean')
    close(bn.running_var, tb.running_var, 1e-2, 1e-3, 'running_var')
    bn.eval()
    tb.eval()
    close(bn(xd.detach(), relu=relu, resid=rd.detach() if res else None),
          (F.relu(tb(xr.detach()) + (rr.detach() if res else 0)) if relu else tb(xr.detach()) + (rr.detach() if res else 0)), 2e-2, 2e-2, 'eval')


def test_maxpool_and_patch_mean():
    from evoke_amd.trunk import _MaxPool, _PatchMean
    x = rnd(2, 12, 10, 64, seed=1)
    x = torch.relu(x)                      # many exact ties at 0, like the real post-ReLU input
    dy = rnd(2, 6, 5, 64, seed=2)
    xd = leaf(x)
    y = _MaxPool.apply(xd)
    y.backward(dy.to(BF).cuda())
    xr = x.to(BF).float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    yr.backward(dy.to(BF).float().permute(0, 3, 1, 2))
    close(y, yr.permute(0, 2, 3, 1), 0, 0, 'maxpool')
    close(xd.grad, xr.grad.permute(0, 2, 3, 1), 1e-2, 1e-2, 'maxpool dx')
    a = rnd(3, 49, 2048, seed=3)
    ad = leaf(a)
    fc = _PatchMean.apply(ad)
    fc.backward(torch.ones_like(fc))
    close(fc, a.to(BF).float().mean(1), 1e-2, 1e-2, 'patch mean')
    close(ad.grad, torch.full_like(a, 1 / 49.0), 1e-2, 1e-4, 'patch mean bwd')


def test_embedding_and_nll():
    from evoke_amd import ops
    Vv, D, B, L = 50, 512, 3, 7
    table, pos = rnd(Vv, D, seed=1), rnd(20, D, seed=2)
    ids = torch.randint(0, Vv, (B, L), generator=torch.Generator().manual_seed(3))
    ids[0, -2:] = 0
    td = table.cuda().requires_grad_(True)
    out = ops.embedding(ids.cuda(), td, pos=pos.cuda(), scale=2.0, padding_idx=0)
    dy = rnd(B, L, D, seed=4)
    out.backward(dy.to(BF).cuda())
    tr = table.clone().requires_grad_(True)
    orf = F.embedding(ids, tr, padding_idx=0) * 2.0 + pos[:L]
    orf.backward(dy.to(BF).float())
    close(out, orf, 1e-2, 1e-2, 'emb')
    close(td.grad, tr.grad, 1e-2, 1e-2, 'demb')
    # masked NLL over padded logits
    Vn, ld = 1445, 1448
    lg = torch.zeros(B * L, ld)
    lg[:, :Vn] = rnd(B * L, Vn, seed=5)
    tgt = torch.randint(0, Vn, (B * L,), generator=torch.Generator().manual_seed(6))
    w = (torch.rand(B * L, generator=torch.Generator().manual_seed(7)) > 0.3).float()
    lgd = lg.cuda().requires_grad_(True)
    loss = ops.nll_loss(lgd, tgt.cuda(), w.cuda(), Vn)
    (loss * 3.0).backward()
    lr = lg[:, :Vn].clone().requires_grad_(True)
    lossr = (-(F.log_softmax(lr, -1).gather(1, tgt[:, None])[:, 0]) * w).sum() / w.sum()
    (lossr * 3.0).backward()
    assert abs(loss.item() - lossr.item()) < 1e-5
    close(lgd.grad[:, :Vn], lr.grad, 1e-2, 1e-4, 'dlogits')
    close(ops.log_softmax(lgd.detach(), Vn), F.log_softmax(lg[:, :Vn], -1), 1e-5, 1e-5, 'log_softmax')


def test_embedding_ids_outside_the_table_never_touch_memory():
    """C ABI: evk_embedding_fwd / evk_embedding_bwd with token ids outside [0, table_rows) -- negative, just past the end, 2^40 -- (a
    corrupted batch, or a stale buffer read by a side stream: the GPU fault of round 3).  Documented behaviour (include/evoke_hip.h): such
    rows are SKIPPED in both directions, the calls return 0 and nothing outside the output / the table gradient is read or written.  The
    table gradient sits between two guard bands that must stay untouched."""
    import ctypes as C
    from evoke_amd import hip as H
    Vv, D, R, L = 40, 64, 12, 4
    table = rnd(Vv, D, seed=11).cuda()
    pos = rnd(L, D, seed=12).cuda()
    ids = torch.tensor([3, -1, Vv, 7, 1 << 40, Vv + 5, 0, -(1 << 33), Vv - 1, 5, -7, 2], dtype=torch.long)
    ok = (ids >= 0) & (ids < Vv)
    out = torch.full((R, D), 7.0, dtype=torch.float32, device='cuda')
    H.check(H.lib.evk_embedding_fwd(H.ptr(table), H.ptr(ids.cuda()), H.ptr(pos), None, H.ptr(out), H.F32, R, D, L, C.c_float(2.0), Vv, None, None,
                                    H.stream()), 'embedding_fwd')
    want = pos.cpu()[torch.arange(R) % L].clone()
    want[ok] += 2.0 * table.cpu()[ids[ok]]
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu(), want, atol=1e-6), 'forward: rows with ids outside the table must hold the positional term only'
    guard = 4096
    buf = torch.full((guard + Vv * D + guard,), 123.0, dtype=torch.float32, device='cuda')
    dtab = buf[guard:guard + Vv * D]
    dtab.zero_()
    dy = rnd(R, D, seed=13).cuda()
    H.check(H.lib.evk_embedding_bwd(H.ptr(dy), H.F32, H.ptr(ids.cuda()), H.ptr(dtab), R, D, C.c_float(0.5), -100, Vv, H.stream()), 'embedding_bwd')
    torch.cuda.synchronize()
    ref = torch.zeros(Vv, D)
    ref.index_add_(0, ids[ok], 0.5 * dy.cpu()[ok])
    assert torch.allclose(dtab.cpu().view(Vv, D), ref, atol=1e-6)
    assert bool((buf[:guard] == 123.0).all()) and bool((buf[guard + Vv * D:] == 123.0).all()), 'backward wrote outside the table gradient'
    # and the malformed CALL (no table rows) is refused with an error code, not launched
    rc = H.lib.evk_embedding_fwd(H.ptr(table), H.ptr(ids.cuda()), H.ptr(pos), None, H.ptr(out), H.F32, R, D, L, C.c_float(1.0), 0, None, None, H.stream())
    assert rc != 0 and b'embedding_fwd' in H.lib.evk_last_error()


@pytest.mark.parametrize('R,ff,cond,split', [(256, False, True, True), (256, False, True, False), (256, True, True, False), (40, True, False, False),
                                             (7, False, True, True), (7, False, True, False), (256, False, None, True), (200, False, False, True),
                                             (256, True, True, True), (40, True, False, True), (7, True, True, True)])
def test_decode_rowblock_projection_residual_and_next_norm(R, ff, cond, split):
    """C ABI: evk_decode_rowblock (csrc/decode_rb.hip) against fp32 torch math on the same 16-bit operands -- output projection / whole
    feed-forward + residual + the next R2Gen (conditional) layer norm (unbiased std, eps on the std: encoder_decoder.py:93-103, 144-179) in
    one launch; row counts that do not fill the last 16-row block; cond None = no norm requested; split = every row block over four workgroups
    that exchange their partial row sums through device memory -- launched THREE times on the same exchange buffer (its arrival counters are
    never reset: each launch must find its own generation)."""
    import ctypes as C
    from evoke_amd import hip as H
    D = 512
    a, x = rnd(R, D, seed=21).to(BF), rnd(R, D, seed=22, scale=2.0).to(BF)                # (rnd is f32: the 16-bit operands are rounded here)
    w1, w2 = rnd(D, D, seed=23, scale=0.06).to(BF), rnd(D, D, seed=24, scale=0.06).to(BF)
    b1, b2 = rnd(D, seed=25, scale=0.1), rnd(D, seed=26, scale=0.1)
    gamma, beta = 1.0 + rnd(D, seed=27, scale=0.1), rnd(D, seed=28, scale=0.1)
    dg, db = rnd(R, D, seed=29, scale=0.2).to(BF), rnd(R, D, seed=30, scale=0.2).to(BF)

    def pack(w):
        out = torch.empty(D * D, dtype=BF, device='cuda')
        H.check(H.lib.evk_decode_rb_pack(H.ptr(w.cuda().contiguous()), H.ptr(out), H.stream()), 'decode_rb_pack')
        return out
    w1p, w2p = pack(w1), pack(w2)
    ad, xd = a.cuda(), x.cuda()
    y = torch.empty(R, D, dtype=BF, device='cuda')
    n = torch.full((R, D), 9.0, dtype=BF, device='cuda')
    b1d, b2d, gd, bd, dgd, dbd = b1.cuda(), b2.cuda(), gamma.cuda(), beta.cuda(), dg.cuda(), db.cuda()
    has_norm = cond is not None
    sync = torch.zeros(H.lib.evk_decode_rowblock_sync_bytes(R), dtype=torch.uint8, device='cuda') if split else None
    for rep in range(3 if split else 1):
        if rep:
            y.fill_(0)
            n.fill_(9.0)
        H.check(H.lib.evk_decode_rowblock(H.ptr(ad), H.ptr(w1p) if ff else None, H.ptr(b1d) if ff else None, H.ptr(w2p), H.ptr(b2d), H.ptr(xd), H.ptr(y),
                                          H.ptr(gd) if has_norm else None, H.ptr(bd) if has_norm else None, H.ptr(dgd) if cond else None,
                                          H.ptr(dbd) if cond else None, D if cond else 0, C.c_float(1e-6), H.ptr(n) if has_norm else None, R,
                                          H.ptr(sync) if split else None, H.stream()), 'decode_rowblock')
    g = a.float()
    if ff:
        g = torch.relu(g @ w1.float().t() + b1).to(BF).float()
    v = x.float() + g @ w2.float().t() + b2
    close(y, v, 4e-3, 4e-3, 'rowblock y')
    if has_norm:
        gg, bb = (gamma + dg.float(), beta + db.float()) if cond else (gamma, beta)
        want = gg * (v - v.mean(-1, keepdim=True)) / (v.std(-1, keepdim=True) + 1e-6) + bb
        close(n, want, 4e-3, 6e-3, 'rowblock norm')
    else:
        assert bool((n == 9.0).all())


@pytest.mark.parametrize('beam,B,f32_mem,last', [(4, 5, True, False), (3, 2, False, False), (4, 3, True, True), (8, 2, False, False), (1, 3, True, False)])
def test_beam_step_kernel_against_the_torch_formulation(beam, B, f32_mem, last):
    """C ABI: evk_beam_step (csrc/beam.hip) against a torch restatement of CaptionModel.beam_search's per-step bookkeeping
    (modules/caption_model.py:51-106 beam_step -- running sum + log-prob, flat DESCENDING sort over beam x (V+1), top-beam, state / sequence
    reorder -- and :174-189 -- [EOS] beams recorded as finished with p = running sum and sent to -1000): selected ids bit-exact including
    TIES (equal scores -> lowest flat index), sequences, cache row table and relational-memory rows permuted in place, best finished beam,
    next tokens, the position advance.  Both kernels behind the entry point are exercised (EVK_BEAM_STEP_FAST is read once per process, so
    the slow one is reached through a vocabulary beyond the fast kernel's register budget)."""
    import ctypes as C
    from evoke_amd import hip as H
    for V1, ld in ((1445, 1448), (1601, 1608)):            # the second: > 24 x 64 candidates per row -> the batched-walk kernel
        max_len, eos, pos0 = 20, V1 - 2, 7
        g = torch.Generator().manual_seed(40 + beam + B)
        logp = torch.log_softmax(torch.randn(B * beam, V1, generator=g) * 2.0, -1)
        logp[:, 50] = logp[:, 900]                                   # ties inside a row ...
        if beam > 1:
            logp[1] = logp[0]                                        # ... and between the first two beams of sample 0 (sums made equal below)
        logp[beam - 1 if B > 1 else 0, eos] = 0.5                    # an [EOS] that wins in sample 0
        lp_pad = torch.full((B * beam, ld), -7.0)
        lp_pad[:, :V1] = logp
        beam_sum = torch.randn(B, beam, generator=g)
        if beam > 1:
            beam_sum[0, 1] = beam_sum[0, 0]
        beam_seq = torch.randint(5, V1 - 3, (B, beam, max_len), generator=g)
        beam_seq[:, :, pos0:] = 0
        best_p = torch.full((B,), -float('inf'))
        best_p[-1] = 1e9                                             # a sample whose earlier finished beam stays the best
        best_seq = torch.randint(5, 50, (B, max_len), generator=g)
        mem_row = 3 * 512 * (2 if f32_mem else 1)                    # in 16-bit units (evk_beam_step's convention)
        mem = torch.randn(B * beam, 3 * 512, generator=g)
        mem = mem if f32_mem else mem.to(BF)
        anc = torch.randint(0, B * beam, (B * beam, max_len), generator=g, dtype=torch.int32)
        d = lambda t: t.clone().cuda()                               # noqa: E731
        lp_d, bs_d, sq_d, bp_d, bq_d, mem_d, anc_d = d(lp_pad), d(beam_sum), d(beam_seq), d(best_p), d(best_seq), d(mem), d(anc)
        words = torch.zeros(B * beam, dtype=torch.long, device='cuda')
        pos = torch.tensor([pos0], dtype=torch.long, device='cuda')
        ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
        H.check(H.lib.evk_beam_step(H.ptr(lp_d), ld, V1, beam, B, max_len, H.ptr(pos), eos, int(last), H.ptr(bs_d), H.ptr(sq_d), H.ptr(bp_d),
                                    H.ptr(bq_d), H.ptr(words), H.ptr(mem_d), mem_row, H.ptr(anc_d), max_len, None if last else H.ptr(pos),
                                    H.ptr(ticket), None, H.stream()), 'beam_step')
        torch.cuda.synchronize()
        # ---- the reference's bookkeeping, restated on the CPU
        cand = (beam_sum.unsqueeze(-1) + logp.view(B, beam, V1)).reshape(B, beam * V1)
        order = torch.sort(cand, dim=1, descending=True, stable=True).indices[:, :beam]          # ties: lowest flat index first
        ys = cand.gather(1, order)
        src, word = order // V1, order % V1
        want_seq = beam_seq.gather(1, src.unsqueeze(-1).expand(-1, -1, max_len)).clone()
        want_seq[:, :, pos0] = word
        rows = (src + torch.arange(B).unsqueeze(1) * beam).reshape(-1)
        want_mem = mem[rows]
        want_anc = anc[rows].clone()
        if not last and pos0 + 1 < max_len:
            want_anc[:, pos0 + 1] = torch.arange(B * beam, dtype=torch.int32)
        end = torch.ones_like(word, dtype=torch.bool) if last else (word == eos)
        want_sum = ys - 1000.0 * end.float()
        want_bp, want_bq = best_p.clone(), best_seq.clone()
        for b in range(B):
            pv, pi = -float('inf'), -1
            for j in range(beam):
                if bool(end[b, j]) and float(ys[b, j]) > pv:
                    pv, pi = float(ys[b, j]), j
            if pi >= 0 and pv > float(want_bp[b]):
                want_bp[b] = pv
                want_bq[b] = want_seq[b, pi]
        assert torch.equal(sq_d.cpu(), want_seq), 'selected sequences differ (V1 = %d)' % V1
        assert torch.equal(words.cpu(), word.reshape(-1))
        assert torch.allclose(bs_d.cpu(), want_sum, atol=1e-5, rtol=0)
        assert torch.equal(mem_d.cpu(), want_mem) and torch.equal(anc_d.cpu(), want_anc)
        assert torch.allclose(bp_d.cpu(), want_bp, atol=1e-5, rtol=0) and torch.equal(bq_d.cpu(), want_bq)
        assert int(pos.item()) == (pos0 if last else pos0 + 1) and int(ticket.item()) == 0
        assert bool(end[0].any()) or last or B == 1                  # the planted [EOS] was selected (the finished-beam branch ran)


@pytest.mark.parametrize('V1', [23, 1537])
def test_beam_step_without_a_comparable_candidate_keeps_every_hypothesis(V1):
    """C ABI: evk_beam_step on a study whose log-probabilities are ALL NaN, next to a finite one.  No candidate of such a study compares, so
    slot r keeps its own hypothesis and emits token 0 at a running sum of -inf: sequences, cache row table and memory rows stay where they
    are (only column pos takes the 0 and column pos + 1 of the row table is seeded), nothing finishes.  Both kernels behind the entry point:
    V1 = 23 takes the register kernel, V1 = 1537 is the smallest vocabulary that takes the batched-walk kernel in an ordinary process (it
    used to form a source row from its sentinel index there).  The finite study is held to the restatement of the test above."""
    from evoke_amd import hip as H
    B, beam, max_len, pos0, mem_row, eos = 2, 3, 8, 3, 8, V1 - 2
    ld = (V1 + 7) // 8 * 8
    g = torch.Generator().manual_seed(77)
    logp = torch.log_softmax(torch.randn(B * beam, V1, generator=g) * 2.0, -1)
    logp[1, eos] = 0.5                                               # an [EOS] that wins in study 0
    logp[beam:] = float('nan')
    lp_pad = torch.full((B * beam, ld), -7.0)
    lp_pad[:, :V1] = logp
    beam_sum = torch.randn(B, beam, generator=g)
    beam_seq = torch.randint(5, V1 - 3, (B, beam, max_len), generator=g)
    beam_seq[:, :, pos0:] = 0
    best_p = torch.full((B,), -float('inf'))
    best_seq = torch.randint(5, V1 - 3, (B, max_len), generator=g)
    mem = torch.randn(B * beam, mem_row, generator=g).to(BF)
    anc = torch.randint(0, B * beam, (B * beam, max_len), generator=g, dtype=torch.int32)
    d = lambda t: t.clone().cuda()                                   # noqa: E731
    lp_d, bs_d, sq_d, bp_d, bq_d, mem_d, anc_d = d(lp_pad), d(beam_sum), d(beam_seq), d(best_p), d(best_seq), d(mem), d(anc)
    words = torch.full((B * beam,), -1, dtype=torch.long, device='cuda')
    pos = torch.tensor([pos0], dtype=torch.long, device='cuda')
    ticket = torch.zeros(1, dtype=torch.int32, device='cuda')
    H.check(H.lib.evk_beam_step(H.ptr(lp_d), ld, V1, beam, B, max_len, H.ptr(pos), eos, 0, H.ptr(bs_d), H.ptr(sq_d), H.ptr(bp_d), H.ptr(bq_d),
                                H.ptr(words), H.ptr(mem_d), mem_row, H.ptr(anc_d), max_len, H.ptr(pos), H.ptr(ticket), None, H.stream()), 'beam_step')
    torch.cuda.synchronize()
    got_seq, got_sum, got_mem, got_anc, got_words = sq_d.cpu(), bs_d.cpu(), mem_d.cpu(), anc_d.cpu().view(B, beam, max_len), words.cpu().view(B, beam)
    seeded = torch.arange(B * beam, dtype=torch.int32).view(B, beam)
    # ---- study 1: nothing compares
    want_seq = beam_seq[1].clone()
    want_seq[:, pos0] = 0
    want_anc = anc.view(B, beam, max_len)[1].clone()
    want_anc[:, pos0 + 1] = seeded[1]
    assert torch.equal(got_seq[1], want_seq) and torch.equal(got_words[1], torch.zeros(beam, dtype=torch.long))
    assert bool((got_sum[1] == -float('inf')).all())
    assert float(bp_d[1]) == -float('inf') and torch.equal(bq_d.cpu()[1], best_seq[1])
    assert torch.equal(got_mem[beam:], mem[beam:]) and torch.equal(got_anc[1], want_anc)
    # ---- study 0: the reference's bookkeeping, restated on the CPU
    cand = (beam_sum[0].unsqueeze(-1) + logp[:beam]).reshape(-1)
    order = torch.sort(cand, descending=True, stable=True).indices[:beam]
    ys, src, word = cand[order], order // V1, order % V1
    want_seq = beam_seq[0][src].clone()
    want_seq[:, pos0] = word
    want_anc = anc.view(B, beam, max_len)[0][src].clone()
    want_anc[:, pos0 + 1] = seeded[0]
    end = word == eos
    assert bool(end.any())                                           # the planted [EOS] was selected
    assert torch.equal(got_seq[0], want_seq) and torch.equal(got_words[0], word)
    assert torch.allclose(got_sum[0], ys - 1000.0 * end.float(), atol=1e-5, rtol=0)
    assert torch.equal(got_mem[:beam], mem[:beam][src]) and torch.equal(got_anc[0], want_anc)
    fin = int(torch.nonzero(end)[0])                                 # (descending: the first finished beam is the best one)
    assert abs(float(bp_d[0]) - float(ys[fin])) <= 1e-5 and torch.equal(bq_d.cpu()[0], want_seq[fin])
    assert int(pos.item()) == pos0 + 1 and int(ticket.item()) == 0


def test_dropout_statistics_and_backward():
    from evoke_amd import ops
    x = torch.ones(1 << 16, dtype=BF).cuda().requires_grad_(True)
    y = ops.dropout(x, 0.3, True)
    keep = (y > 0).float().mean().item()
    assert abs(keep - 0.7) < 0.01
    assert abs(float(y.float().max()) - 1 / 0.7) < 1e-2
    y.backward(torch.ones_like(y))
    assert torch.equal((x.grad > 0), (y > 0))
    r = torch.full_like(x, 2.0).detach().requires_grad_(True)
    z = ops.dropout(x.detach().requires_grad_(True), 0.5, True, resid=r)
    assert float(z.float().min()) == 2.0 and float(z.float().max()) == 4.0


def test_contrastive_losses_match_oracle():
    from evoke_amd import losses
    from evoke_amd import ops
    from oracle import functional as O
    sc = ops.loss_scale_value()          # fp16 storage: back-propagate under the model-level loss scale, compare grad / scale
    pid = np.array(['a', 'b', 'c', 'a', 'c', 'a'])
    g = rnd(6, 2048, seed=1)
    gd = g.cuda().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    l, lr_ = losses.multi_pos_contra_images(gd, pid, 0.5), O.multi_pos_contra_images(gr, pid, 0.5)
    ops.scale_loss(l).backward(); lr_.backward()
    assert abs(l.item() - lr_.item()) < 2e-5, (l.item(), lr_.item())
    close(gd.grad / sc, gr.grad, 2e-3, 1e-6, 'multi_pos grad')
    assert tuple(losses.multi_pos_contra_images(gd, np.array(list('abcdef')), 0.5).shape) == (1,)
    v, t = rnd(3, 2048, seed=2), rnd(3, 2048, seed=3)
    vd, td = v.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
    vr, tr = v.clone().requires_grad_(True), t.clone().requires_grad_(True)
    l, lr_ = losses.global_alignment(vd, td, pid, 0.5), O.global_alignment_loss(vr, tr, pid, 0.5)
    ops.scale_loss(l).backward(); lr_.backward()
    assert abs(l.item() - lr_.item()) < 2e-5, (l.item(), lr_.item())
    close(vd.grad / sc, vr.grad, 2e-3, 1e-6, 'global grad v')
    close(td.grad / sc, tr.grad, 2e-3, 1e-6, 'global grad t')
    p, tk = rnd(3, 49, 2048, seed=4), rnd(3, 9, 2048, seed=5)
    pd, tkd = p.cuda().requires_grad_(True), tk.cuda().requires_grad_(True)
    pr, tkr = p.clone().requires_grad_(True), tk.clone().requires_grad_(True)
    l, lr_ = losses.local_text_token_alignment(pd, tkd, 0.5), O.local_text_token_alignment_loss(pr, tkr, 0.5)
    ops.scale_loss(l).backward(); lr_.backward()
    assert abs(l.item() - lr_.item()) < 2e-5, (l.item(), lr_.item())
    close(pd.grad / sc, pr.grad, 5e-3, 1e-7, 'local grad p')
    close(tkd.grad / sc, tkr.grad, 5e-3, 1e-7, 'local grad t')


@pytest.mark.parametrize('B,L,persistent', [(2, 5, 1), (3, 12, 0), (3, 12, 1), (2, 100, 1)])
def test_relational_memory_step_matches_oracle(B, L, persistent):
    """RelationalMemory.forward (encoder_decoder.py:263-300) + BPTT against the fp32 oracle: the per-token launch sequence
    (L < 8 or persistent off) and the persistent one-launch-per-direction kernels (csrc/rm.hip), up to max_seq_len = 100 tokens."""
    from evoke_amd import hip as H, ops
    from evoke_amd.layers import RelationalMemory
    from oracle import functional as O
    ops.set_dropout_enabled(False)
    H.check(H.lib.evk_rm_set_persistent(persistent))
    torch.manual_seed(3)
    rm = RelationalMemory(3, 512, 8).cuda().train()
    P = {'text_decoder.model.rm.' + k: v.detach().cpu().to(BF).float() if v.dim() > 1 else v.detach().cpu().clone()
         for k, v in rm.state_dict().items()}
    for k in P:
        P[k].requires_grad_(True)
    emb = rnd(B, L, 512, seed=1)
    ed = leaf(emb)
    out = rm(ed)
    gsc = 1.0 / L                                   # keep the summed gradient O(1) for long walks
    (out.float().sum() * gsc).backward()
    er = ref(emb)
    cfg = dict(rm_num_slots=3, rm_d_model=512, rm_num_heads=8)
    outr = O.rm_forward(P, er, cfg, O.Ctx(train=True))
    (outr.sum() * gsc).backward()
    ops.set_dropout_enabled(True)
    H.check(H.lib.evk_rm_set_persistent(0))
    from tests.helpers import rel_err
    if L <= 20:
        close(out, outr, 3e-2, 3e-2, 'rm out')
        close(ed.grad, er.grad, 8e-2, 8e-2, 'rm demb')
        close(rm.W.weight.grad, P['text_decoder.model.rm.W.weight'].grad, 8e-2, 8e-2, 'rm dW')
    else:       # 100 recurrent tokens in 16-bit storage: single elements drift (measured max 0.11 at rel-norm 2.6e-3): compare by norm
        e_out, e_emb, e_w = rel_err(out, outr), rel_err(ed.grad, er.grad), rel_err(rm.W.weight.grad, P['text_decoder.model.rm.W.weight'].grad)
        print('   rm L=%d rel-norm err: out %.2e demb %.2e dW %.2e' % (L, e_out, e_emb, e_w))
        # bf16 storage (8-bit mantissa) through 100 recurrent tokens measures 4e-2 / 0.33 / 0.32: the recurrence amplifies storage rounding
        lim = (1e-2, 5e-2, 5e-2) if F16_BUILD else (8e-2, 0.5, 0.5)
        assert e_out <= lim[0] and e_emb <= lim[1] and e_w <= lim[2], (e_out, e_emb, e_w)
    # the other recurrence weights by relative norm (a 16-bit forward flips a few ReLU gates of the memory MLP: point-wise
    # differences on single elements, energy-wise small)
    for what, got, key in (('dU', rm.U.weight.grad, 'U.weight'), ('dWq', rm.attn.linears[0].weight.grad, 'attn.linears.0.weight'),
                           ('dWo', rm.attn.linears[3].weight.grad, 'attn.linears.3.weight'), ('dW0', rm.mlp[0].weight.grad, 'mlp.0.weight'),
                           ('dW2', rm.mlp[2].weight.grad, 'mlp.2.weight')):
        e = rel_err(got, P['text_decoder.model.rm.' + key].grad)
        print('   rm %-4s rel-norm err %.2e' % (what, e))
        assert e <= (5e-2 if (F16_BUILD or L <= 20) else 0.5), (what, e)


def test_relational_memory_persistent_kernels_match_the_launch_sequence():
    """The persistent kernels round every intermediate to 16 bits at the same points as the per-token launch path, so the two
    differ only by the f32 summation order inside the GEMMs: outputs and input gradients agree to a few 16-bit ulps, with the
    dropout of the memory attention ON (both draw the same stateless-hash masks)."""
    from evoke_amd import hip as H, ops
    from evoke_amd.layers import RelationalMemory
    torch.manual_seed(4)
    rm = RelationalMemory(3, 512, 8).cuda().train()
    emb = rnd(4, 24, 512, seed=2)
    res = []
    for persistent in (0, 1):
        H.check(H.lib.evk_rm_set_persistent(persistent))
        ops.manual_seed(99)
        for prm in rm.parameters():
            prm.grad = None
        ed = leaf(emb)
        out = rm(ed)
        (out.float() * rnd(4, 24, 1536, seed=5).cuda()).sum().backward()
        res.append((out.detach().float().cpu(), ed.grad.detach().float().cpu(), rm.mlp[2].weight.grad.detach().cpu().clone(),
                    rm.attn.linears[1].weight.grad.detach().cpu().clone()))
    H.check(H.lib.evk_rm_set_persistent(0))
    for a, b, what in zip(res[0], res[1], ('out', 'demb', 'dW2', 'dWk')):
        err = float((a - b).abs().max() / (a.abs().max() + 1e-12))
        print('   persistent vs launch path %-5s rel max err %.2e' % (what, err))
        assert err < 2e-2, (what, err)


def test_optim_step_matches_torch():
    import ctypes as C
    from evoke_amd import hip as H
    n = 1000
    for kind, mk in ((0, lambda p: torch.optim.RAdam(p, lr=5e-3, weight_decay=1e-4)),
                     (1, lambda p: torch.optim.Adam(p, lr=5e-3, weight_decay=1e-4, amsgrad=True))):
        p0, gs = rnd(n, seed=1), [rnd(n, seed=10 + i, scale=0.3) for i in range(8)]
        pr = p0.clone().requires_grad_(True)
        opt = mk([pr])
        pd = p0.clone().cuda()
        m, v, vm = torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
        sh = torch.zeros(n, dtype=BF).cuda()
        for step, g in enumerate(gs, 1):
            pr.grad = g.clamp(-0.1, 0.1)
            opt.step()
            H.check(H.lib.evk_optim_step(H.ptr(pd), H.ptr(g.cuda()), H.ptr(m), H.ptr(v), H.ptr(vm) if kind == 1 else None, H.ptr(sh), n,
                                         kind, 5e-3, 0.9, 0.999, 1e-8, 1e-4, 0.1, step, H.stream()))
        close(pd, pr, 1e-5, 1e-6, 'optim kind %d' % kind)
        close(sh, pr, 1e-2, 1e-3, 'shadow')
        # loss-scaled gradients (x 1024) with grad_scale = 1/1024 take the same steps; a non-finite gradient skips its element
        pd2 = p0.clone().cuda()
        m2, v2, vm2 = torch.zeros(n).cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
        for step, g in enumerate(gs, 1):
            gsc = (g * 1024.0).cuda()
            gsc[7] = float('inf')
            H.check(H.lib.evk_optim_step_scaled(H.ptr(pd2), H.ptr(gsc), H.ptr(m2), H.ptr(v2), H.ptr(vm2) if kind == 1 else None, None, n,
                                                kind, 5e-3, 0.9, 0.999, 1e-8, 1e-4, 0.1, step, 1.0 / 1024.0, H.stream()))
        keep = torch.ones(n, dtype=torch.bool)
        keep[7] = False
        close(pd2.cpu()[keep], pd.cpu()[keep], 1e-6, 1e-7, 'scaled optim kind %d' % kind)
        assert float(pd2[7]) == float(p0[7]) and float(m2[7]) == 0.0


@pytest.mark.parametrize('kind', [0, 1])
def test_optim_group_step_per_parameter_counts_and_device_hyperparameters(kind):
    """evk_optim_group_step through the C ABI: one flat group of five parameters (sizes that are not multiples of the 8-element padding)
    against torch.optim.RAdam / Adam(amsgrad) run PER PARAMETER: the parameters join in at different steps and sit some steps out (the
    touched mask), so their step counts differ inside one launch; the learning rate changes half way through by rewriting the device
    buffer only; a step with the overflow flag set moves nothing and advances no count; gradients arrive scaled by 512 and summed over a
    world of 2 and are consumed (zeroed) by the kernel."""
    import ctypes as C
    from evoke_amd import hip as H
    sizes = [37, 1024, 8, 4099, 640]
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += (n + 7) // 8 * 8
    g = torch.Generator().manual_seed(4)
    p0 = [torch.randn(n, generator=g) for n in sizes]
    ref = [torch.nn.Parameter(t.clone()) for t in p0]
    mk = (lambda ps, lr: torch.optim.RAdam(ps, lr=lr, weight_decay=1e-4)) if kind == 0 else (lambda ps, lr: torch.optim.Adam(ps, lr=lr, weight_decay=1e-4, amsgrad=True))
    ropt = [mk([q], 5e-3) for q in ref]
    flat = {k: torch.zeros(tot, device='cuda') for k in ('p', 'g', 'm', 'v', 'vm')}
    sh = torch.zeros(tot, dtype=BF, device='cuda')
    for t, o in zip(p0, offs):
        flat['p'][o:o + t.numel()] = t.cuda()
    steps = torch.zeros(len(sizes), dtype=torch.int32, device='cuda')
    offs_dev = torch.tensor(offs, dtype=torch.int64, device='cuda')
    coef = torch.zeros(4 * len(sizes), device='cuda')
    hp = torch.tensor([5e-3, 0.9, 0.999, 1e-8, 1e-4, 0.1, 0, 0], dtype=torch.float32, device='cuda')
    state = torch.tensor([512.0, 0.0, 0.0, 0.0], device='cuda')
    masks = [[1, 1, 0, 1, 0], [1, 0, 0, 1, 0], [1, 1, 0, 1, 0], [0, 1, 1, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [1, 0, 1, 1, 1], [1, 1, 1, 1, 1],
             [1, 1, 1, 1, 1], [1, 1, 0, 1, 1]]
    for it, mask in enumerate(masks):
        if it == 4:                                             # an lr scheduler: only the device buffer changes
            hp[0] = 1e-3
            for o in ropt:
                o.param_groups[0]['lr'] = 1e-3
        overflow = it == 6
        state[2] = 1.0 if overflow else 0.0
        for i, (q, o) in enumerate(zip(ref, offs)):
            gi = torch.randn(sizes[i], generator=g) * 0.2
            if mask[i]:
                flat['g'][o:o + sizes[i]] = (gi * 512.0 * 2.0).cuda()         # loss scale x sum over 2 ranks
                if not overflow:
                    q.grad = gi.clamp(-0.1, 0.1)
                    ropt[i].step()
        m = torch.tensor(mask, dtype=torch.uint8, device='cuda')
        H.check(H.lib.evk_optim_group_step(H.ptr(flat['p']), H.ptr(flat['g']), H.ptr(flat['m']), H.ptr(flat['v']), H.ptr(flat['vm']) if kind == 1 else None,
                                           H.ptr(sh), tot, kind, H.ptr(hp), H.ptr(offs_dev), len(sizes), H.ptr(steps), H.ptr(m), H.ptr(coef), H.ptr(state),
                                           C.c_float(0.5), 1, H.stream()))
        assert float(flat['g'].abs().sum()) == 0.0, 'gradients of the touched parameters are consumed'
    want_steps = [sum(mk_[i] for j, mk_ in enumerate(masks) if j != 6) for i in range(len(sizes))]
    assert steps.cpu().tolist() == want_steps, (steps.cpu().tolist(), want_steps)
    assert len(set(want_steps)) > 2                                   # the counts really differ inside the one launch
    for i, (q, o) in enumerate(zip(ref, offs)):
        close(flat['p'][o:o + sizes[i]], q.detach(), 2e-5, 2e-6, 'parameter %d (kind %d)' % (i, kind))
        close(sh[o:o + sizes[i]].float(), q.detach(), 1e-2, 1e-3, 'shadow %d' % i)


def test_rm_decode_step_is_bit_identical_to_the_recurrence_runner():
    """evk_rm_decode_step (one generated token of the relational memory: 8 launches, state in place) against evk_rm_forward with L = 1 fed
    with the three hoisted projections (what RelationalMemory.run does): same kernels, same arithmetic -> torch.equal on the new memory,
    on tanh(memory) and on the memory row handed to the decoder, over three consecutive tokens."""
    import ctypes as C
    from evoke_amd import hip as H, ops
    from evoke_amd.layers import RelationalMemory
    torch.manual_seed(2)
    rm = RelationalMemory(3, 512, 8).cuda().eval()
    B = 24
    lin = rm.attn.linears
    wx = torch.cat([lin[1].weight, lin[2].weight, rm.W.weight], 0).detach().to(BF).contiguous()
    bx = torch.cat([lin[1].bias, lin[2].bias, rm.W.bias], 0).detach().float().contiguous()
    wqkv = torch.cat([lin[i].weight for i in range(3)], 0).detach().to(BF).contiguous()
    bqkv = torch.cat([lin[i].bias for i in range(3)], 0).detach().float().contiguous()
    rest = [(m.weight.detach().to(BF).contiguous(), m.bias.detach().float().contiguous()) for m in (lin[3], rm.mlp[0], rm.mlp[2], rm.U)]
    mem = rm.init_memory(B, 'cuda')
    mem_b = mem.clone()
    tmem = torch.empty_like(mem_b)
    H.check(H.lib.evk_act_fwd(H.ptr(mem_b), H.ptr(tmem), mem_b.numel(), H.ACT_TANH, H.stream()))
    ws = torch.empty(H.lib.evk_rm_decode_ws_bytes(B), dtype=torch.uint8, device='cuda')
    out_b = torch.empty(B, 1, 1536, dtype=BF, device='cuda')
    with torch.no_grad():
        for t in range(3):
            emb = (torch.randn(B, 1, 512, device='cuda') * 0.8).to(BF)
            out_a, mem = rm.run(emb, mem)
            (wo, bo), (w0, b0), (w2, b2), (wu, bu) = rest
            H.check(H.lib.evk_rm_decode_step(H.ptr(emb), H.ptr(wx), H.ptr(bx), H.ptr(mem_b), H.ptr(tmem), H.ptr(wqkv), H.ptr(bqkv), H.ptr(wo), H.ptr(bo),
                                             H.ptr(w0), H.ptr(b0), H.ptr(w2), H.ptr(b2), H.ptr(wu), H.ptr(bu), H.ptr(out_b), H.ptr(ws), ws.numel(), B,
                                             H.stream()))
            assert torch.equal(mem.reshape(-1), mem_b.reshape(-1)), 'memory after token %d' % t
            assert torch.equal(out_a.reshape(-1), out_b.reshape(-1)), 'memory row after token %d' % t
            assert torch.equal(tmem.float(), torch.tanh(mem_b.float()).to(BF).float()) or (tmem.float() - torch.tanh(mem_b.float())).abs().max() < 2e-3


@pytest.mark.parametrize('split', [0, 1])
def test_rm_decode_step_f32_follows_the_fp32_oracle_through_a_long_recurrence(split):
    """evk_rm_decode_step_f32 (the decode step's relational memory: f32 masters, f32 state, products on the f32-input MFMA -- split 0 -- or
    as three fp16 MFMAs over hi / lo halves of the f32 operands -- split 1, opt-in in the fp16 build, evk_rm_f32_split16) against the
    oracle's rm_step (CPU restatement of modules/encoder_decoder.py:274-291) over 60 consecutive tokens from the same inputs.  The
    recurrence amplifies rounding (that is why it runs in f32), so the yardstick is the oracle itself: run in float64 it is the truth,
    run in float32 it shows what f32 arithmetic can do; the engine must stay within 4 x the f32 oracle's own distance from the truth
    (+ 1e-5) on the f32 MFMA and within 8 x with split operands (2^-22 per operand against 2^-24; measured 4.9 x; the 16-bit recurrence
    this path replaced: > 1000 x).  The 16-bit row handed to the decoder must be the memory rounded."""
    from evoke_amd import hip as H
    from evoke_amd.layers import RelationalMemory
    from oracle import functional as O
    before = H.lib.evk_rm_f32_split16(-1)
    if H.lib.evk_rm_f32_split16(split) != split:
        H.lib.evk_rm_f32_split16(before)
        pytest.skip('this build forms the products on the f32 MFMA only')
    try:
        _rm_recurrence_against_the_oracles(H, RelationalMemory, O, 8 if split else 4)
    finally:
        H.lib.evk_rm_f32_split16(before)


def _rm_recurrence_against_the_oracles(H, RelationalMemory, O, factor):
    torch.manual_seed(6)
    rm = RelationalMemory(3, 512, 8).cuda().eval()
    with torch.no_grad():
        for prm in rm.parameters():                      # a lively recurrence: larger weights than the Xavier init
            if prm.dim() > 1:
                prm.mul_(1.6)
    pre = 'text_decoder.model.rm'
    names = {'attn.linears.0': rm.attn.linears[0], 'attn.linears.1': rm.attn.linears[1], 'attn.linears.2': rm.attn.linears[2],
             'attn.linears.3': rm.attn.linears[3], 'mlp.0': rm.mlp[0], 'mlp.2': rm.mlp[2], 'W': rm.W, 'U': rm.U}
    P = {}
    for k, m in names.items():
        P['%s.%s.weight' % (pre, k)] = m.weight.detach().float().cpu()
        P['%s.%s.bias' % (pre, k)] = m.bias.detach().float().cpu()
    cfg = dict(O.DEFAULT_CFG)
    B = 5
    lin = rm.attn.linears
    f = lambda t: t.detach().float().contiguous()          # noqa: E731
    wx, bx = f(torch.cat([lin[1].weight, lin[2].weight, rm.W.weight], 0)), f(torch.cat([lin[1].bias, lin[2].bias, rm.W.bias], 0))
    wqkv, bqkv = f(torch.cat([lin[i].weight for i in range(3)], 0)), f(torch.cat([lin[i].bias for i in range(3)], 0))
    rest = [(f(m.weight), f(m.bias)) for m in (lin[3], rm.mlp[0], rm.mlp[2], rm.U)]
    mem = rm.init_memory(B, 'cuda').float().contiguous()
    ref = O.rm_init_memory(B, 3, 512).reshape(B, -1)
    P64 = {k: v.double() for k, v in P.items()}
    ref64 = ref.double()
    ws = torch.empty(H.lib.evk_rm_decode_f32_ws_bytes(B), dtype=torch.uint8, device='cuda')
    out16 = torch.empty(B, 1536, dtype=BF, device='cuda')
    g = torch.Generator().manual_seed(8)
    worst = worst32 = 0.0
    with torch.no_grad():
        for t in range(60):
            x = torch.randn(B, 512, generator=g) * 0.9
            ref = O.rm_step(P, x, ref, cfg, O.Ctx())
            ref64 = O.rm_step(P64, x.double(), ref64, cfg, O.Ctx())
            worst32 = max(worst32, float((ref.double() - ref64).abs().max()))
            xd = x.cuda().contiguous()
            (wo, bo), (w0, b0), (w2, b2), (wu, bu) = rest
            H.check(H.lib.evk_rm_decode_step_f32(H.ptr(xd), H.ptr(wx), H.ptr(bx), H.ptr(mem), H.ptr(wqkv), H.ptr(bqkv), H.ptr(wo), H.ptr(bo), H.ptr(w0),
                                                 H.ptr(b0), H.ptr(w2), H.ptr(b2), H.ptr(wu), H.ptr(bu), H.ptr(out16), H.ptr(ws), ws.numel(), B, H.stream()))
            err = float((mem.reshape(B, -1).cpu().double() - ref64).abs().max())
            worst = max(worst, err)
            assert torch.equal(out16.float().cpu(), mem.reshape(B, -1).to(BF).float().cpu())
    print('\n[f32 relational memory] max |memory - float64 oracle| over 60 tokens: engine %.2e, float32 oracle %.2e' % (worst, worst32))
    assert worst <= factor * worst32 + 1e-5, (worst, worst32)


def test_conv_fwd_stats_and_dgrad_add():
    """conv epilogue batch-norm statistics (evk_conv2d_fwd_stats + evk_bn_stats_from_partials) and the fused skip-gradient
    add of the data gradient (evk_conv2d_dgrad_add) against f32 torch convolutions of the same bf16 operands."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(3)
    for (N, Hh, Ci, Co, k, stride) in [(3, 20, 64, 128, 3, 1), (2, 24, 128, 64, 1, 1), (2, 18, 64, 256, 3, 2), (5, 12, 256, 1024, 1, 1),
                                     (1, 513, 64, 256, 1, 1)]:       # last: 263k ragged rows (1029 row blocks of statistics partials)
        g = H.conv_geom(N, Hh, Hh, Ci, Co, k, k, stride, k // 2)
        x = (torch.randn(N, Hh, Hh, Ci, device='cuda') * 0.7).to(BF)
        w = (torch.randn(Co, k, k, Ci, device='cuda') * 0.05).to(BF)
        y = torch.empty(N, g.Ho, g.Wo, Co, device='cuda', dtype=BF)
        M = N * g.Ho * g.Wo
        nb = H.lib.evk_conv_stats_bytes(M, Co)
        part = torch.empty(nb // 4, device='cuda')
        nblk = C.c_int32(0)
        H.check(H.lib.evk_conv2d_fwd_stats(H.ptr(x), H.ptr(w), H.ptr(y), C.byref(g), H.ptr(part), nb, C.byref(nblk), H.stream()))
        st = torch.empty(2, Co, device='cuda')
        H.check(H.lib.evk_bn_stats_from_partials(H.ptr(part), nblk.value, H.ptr(st[0]), H.ptr(st[1]), Co, H.stream()))
        ref = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), stride=stride, padding=k // 2).permute(0, 2, 3, 1)
        ref = ref.cpu()
        close(y.float(), ref, 1e-2, 2e-2, 'conv y')
        close(st[0], ref.reshape(-1, Co).sum(0), 2e-3, 2e-3 * float(ref.abs().sum(dim=(0, 1, 2)).max()), 'stats sum')
        close(st[1], (ref.reshape(-1, Co) ** 2).sum(0), 2e-3, 1e-3, 'stats sumsq')
        dy = (torch.randn(N, g.Ho, g.Wo, Co, device='cuda') * 0.3).to(BF)
        skip = (torch.randn(N, Hh, Hh, Ci, device='cuda') * 0.3).to(BF)
        dx = torch.empty(N, Hh, Hh, Ci, device='cuda', dtype=BF)
        H.check(H.lib.evk_conv2d_dgrad_add(H.ptr(dy), H.ptr(w), H.ptr(skip), H.ptr(dx), C.byref(g), H.stream()))
        xr = x.float().permute(0, 3, 1, 2).requires_grad_(True)
        torch.nn.functional.conv2d(xr, w.float().permute(0, 3, 1, 2), stride=stride, padding=k // 2).backward(dy.float().permute(0, 3, 1, 2))
        close(dx.float(), (xr.grad.permute(0, 2, 3, 1) + skip.float()).cpu(), 2e-2, 2e-2, 'dgrad + skip')


def helpers_f16():
    from tests.helpers import F16_BUILD
    return F16_BUILD


def test_dgrad_gate_statistics_give_the_batchnorm_backward_sums():
    """evk_conv2d_dgrad_gated_stats + evk_bn_bwd_sums_from_gate_partials: the data-gradient GEMM's epilogue accumulates sum(g) and
    sum(g*z) of its ReLU-gated output per channel (z = relu(gamma*xhat + beta), the gate tensor), from which the batch-norm backward
    sums sum(g) and sum(g*xhat) of that layer follow without a pass over g -- against f32 torch on the same 16-bit operands."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(5)
    for (N, Hh, Ci, Co, k, stride) in [(3, 20, 64, 128, 3, 1), (2, 24, 256, 64, 1, 1), (2, 18, 128, 256, 3, 2), (1, 257, 64, 256, 1, 1)]:
        g = H.conv_geom(N, Hh, Hh, Ci, Co, k, k, stride, k // 2)
        M = N * Hh * Hh
        w = (torch.randn(Co, k, k, Ci, device='cuda') * 0.05).to(BF)
        dy = (torch.randn(N, g.Ho, g.Wo, Co, device='cuda') * 0.3).to(BF)
        gamma, beta = 0.5 + torch.rand(Ci, device='cuda'), 0.3 * torch.randn(Ci, device='cuda')
        xhat = torch.randn(N, Hh, Hh, Ci, device='cuda')
        z = torch.relu(gamma * xhat + beta).to(BF)                   # the layer's forward output = the gate
        dx = torch.empty(N, Hh, Hh, Ci, device='cuda', dtype=BF)
        nb = H.lib.evk_conv_stats_bytes(M, Ci)
        part = torch.empty(nb // 4, device='cuda')
        nblk = C.c_int32(0)
        H.check(H.lib.evk_conv2d_dgrad_gated_stats(H.ptr(dy), H.ptr(w), None, H.ptr(z), H.ptr(dx), C.byref(g), H.ptr(part), nb, C.byref(nblk), H.stream()))
        sums = torch.empty(2, Ci, device='cuda')
        dbeta, dgamma = torch.ones(Ci, device='cuda'), torch.ones(Ci, device='cuda')
        H.check(H.lib.evk_bn_bwd_sums_from_gate_partials(H.ptr(part), nblk.value, H.ptr(gamma), H.ptr(beta), H.ptr(sums[0]), H.ptr(sums[1]),
                                                         H.ptr(dbeta), H.ptr(dgamma), Ci, None, None, None, None, 0, H.stream()))
        xr = torch.zeros(N, Ci, Hh, Hh, device='cuda', requires_grad=True)
        torch.nn.functional.conv2d(xr, w.float().permute(0, 3, 1, 2), stride=stride, padding=k // 2).backward(dy.float().permute(0, 3, 1, 2))
        gref = (xr.grad.permute(0, 2, 3, 1) * (z.float() > 0)).reshape(-1, Ci)
        zf = z.float().reshape(-1, Ci)
        xh = (zf - beta) / gamma                                      # xhat as the gate lets it be recovered (where z > 0)
        want_g, want_gx = gref.sum(0).cpu(), (gref * xh).sum(0).cpu()
        scale = float(gref.abs().sum(0).max())
        close(dx.float().reshape(-1, Ci), gref.cpu(), 2e-2, 2e-2, 'gated dgrad')
        close(sums[0], want_g, 5e-3, 5e-3 * scale, 'sum g')
        close(sums[1], want_gx, 5e-3, 1e-2 * scale, 'sum g*xhat')
        close(dbeta - 1, want_g, 5e-3, 5e-3 * scale, 'dbeta acc')


def test_flipped_weight_data_gradient_matches_the_gather_kernel_and_torch():
    """evk_conv_flip_weights + evk_conv2d_dgrad_flipped_gated_stats: the data gradient of a stride-1 3x3 convolution run as a forward
    convolution of dy with flipped / transposed weights -- against the gather formulation (evk_conv2d_dgrad_gated_stats: same gate, same
    statistics) and f32 torch, on shapes with ragged row tiles and several layers in one flip launch."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(9)
    shapes = [(2, 24, 256, 256), (3, 10, 64, 64), (1, 31, 128, 128), (2, 12, 512, 512)]
    ws = [(torch.randn(co, 3, 3, ci, device='cuda') * 0.05).to(BF) for (_, _, ci, co) in shapes]
    wts = [torch.empty(ci, 3, 3, co, device='cuda', dtype=BF) for (_, _, ci, co) in shapes]
    n = len(shapes)
    arr = lambda vals, ty: (ty * n)(*vals)          # noqa: E731
    H.check(H.lib.evk_conv_flip_weights(arr([H.ptr(w) for w in ws], C.c_void_p), arr([H.ptr(w) for w in wts], C.c_void_p),
                                        arr([s[3] for s in shapes], C.c_int32), arr([s[2] for s in shapes], C.c_int32), arr([3] * n, C.c_int32),
                                        arr([3] * n, C.c_int32), n, H.stream()))
    for (N, Hh, Ci, Co), w, wt in zip(shapes, ws, wts):
        assert torch.equal(wt, w.flip(1, 2).permute(3, 1, 2, 0).contiguous()), 'flip kernel'
        g = H.conv_geom(N, Hh, Hh, Ci, Co, 3, 3, 1, 1)
        M = N * Hh * Hh
        dy = (torch.randn(N, Hh, Hh, Co, device='cuda') * 0.3).to(BF)
        z = torch.relu(torch.randn(N, Hh, Hh, Ci, device='cuda')).to(BF)
        nb = H.lib.evk_conv_stats_bytes(M, Ci)
        outs = []
        for flipped in (False, True):
            dx = torch.empty(N, Hh, Hh, Ci, device='cuda', dtype=BF)
            part = torch.zeros(nb // 4, device='cuda')
            nblk = C.c_int32(0)
            fn = H.lib.evk_conv2d_dgrad_flipped_gated_stats if flipped else H.lib.evk_conv2d_dgrad_gated_stats
            H.check(fn(H.ptr(dy), H.ptr(wt if flipped else w), None, H.ptr(z), H.ptr(dx), C.byref(g), H.ptr(part), nb, C.byref(nblk), H.stream()))
            sums = part[:nblk.value * 2 * Ci].view(nblk.value, 2, Ci).sum(0)
            outs.append((dx, sums))
        xr = torch.zeros(N, Ci, Hh, Hh, device='cuda', requires_grad=True)
        torch.nn.functional.conv2d(xr, w.float().permute(0, 3, 1, 2), stride=1, padding=1).backward(dy.float().permute(0, 3, 1, 2))
        gref = xr.grad.permute(0, 2, 3, 1) * (z.float() > 0)
        scale = float(gref.abs().reshape(-1, Ci).sum(0).max())
        close(outs[1][0].float(), gref.cpu(), 2e-2, 2e-2, 'flipped dgrad vs torch')
        close(outs[1][0].float(), outs[0][0].float().cpu(), 1e-2, 1e-2, 'flipped vs gather dgrad')
        close(outs[1][1][0], gref.reshape(-1, Ci).sum(0).cpu(), 5e-3, 5e-3 * scale, 'sum g')
        close(outs[1][1][1], (gref * z.float()).reshape(-1, Ci).sum(0).cpu(), 5e-3, 1e-2 * scale, 'sum g*z')


@pytest.mark.parametrize('tiny', [1e-2, 1e-4, 1e-6])
def test_gate_statistics_fall_back_to_exact_sums_for_near_dead_channels(tiny):
    """ImageNet-pretrained resnet101 has batch-norm channels with |gamma| << |beta|.  There xhat = (z - beta) / gamma amplifies the 16-bit
    rounding of the stored z by |beta / gamma| and the gate-statistic dgamma would be noise; evk_bn_bwd_sums_from_gate_partials recomputes
    such channels exactly (from the gated gradient and the raw convolution output) inside the same launch.  Channels 0-7 and 40-47 get
    gamma = `tiny` with beta = 0.5; the rest stay well conditioned.  Against an f32 batch-norm backward; the fallback switched off (dz =
    NULL) must show the error it removes."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(7)
    N, Hh, Ci, Co = 2, 24, 64, 128
    M = N * Hh * Hh
    g = H.conv_geom(N, Hh, Hh, Ci, Co, 1, 1, 1, 0)
    w = (torch.randn(Co, 1, 1, Ci, device='cuda') * 0.05).to(BF)
    dy = (torch.randn(N, Hh, Hh, Co, device='cuda') * 0.3).to(BF)
    gamma, beta = 0.5 + torch.rand(Ci, device='cuda'), 0.3 * torch.randn(Ci, device='cuda')
    dead = list(range(0, 8)) + list(range(40, 48))
    gamma[dead], beta[dead] = tiny, 0.5
    y = (torch.randn(N, Hh, Hh, Ci, device='cuda') * 1.7 + 0.4).to(BF)          # the layer's raw convolution output
    yf = y.float().reshape(-1, Ci)
    mean, var = yf.mean(0), yf.var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    xhat = (yf - mean) * invstd
    z = torch.relu(gamma * xhat + beta).reshape(N, Hh, Hh, Ci).to(BF)
    dx = torch.empty(N, Hh, Hh, Ci, device='cuda', dtype=BF)
    nb = H.lib.evk_conv_stats_bytes(M, Ci)
    part = torch.empty(nb // 4, device='cuda')
    nblk = C.c_int32(0)
    H.check(H.lib.evk_conv2d_dgrad_gated_stats(H.ptr(dy), H.ptr(w), None, H.ptr(z), H.ptr(dx), C.byref(g), H.ptr(part), nb, C.byref(nblk), H.stream()))
    gated = dx.float().reshape(-1, Ci)                                             # what the fallback reads
    want = (gated * xhat).sum(0)
    scale = float((gated.abs() * xhat.abs()).sum(0).max())

    def run(fallback):
        sums = torch.empty(2, Ci, device='cuda')
        dgamma = torch.zeros(Ci, device='cuda')
        args = (H.ptr(dx), H.ptr(y), H.ptr(mean), H.ptr(invstd), M) if fallback else (None, None, None, None, 0)
        H.check(H.lib.evk_bn_bwd_sums_from_gate_partials(H.ptr(part), nblk.value, H.ptr(gamma), H.ptr(beta), H.ptr(sums[0]), H.ptr(sums[1]), None,
                                                         H.ptr(dgamma), Ci, *args, H.stream()))
        assert torch.equal(sums[1], dgamma)
        return dgamma

    got, raw = run(True), run(False)
    err = ((got - want).abs() / scale).cpu()
    err_raw = ((raw - want).abs() / scale).cpu()
    print('\n[near-dead BN channels, gamma = %g] relative error of dgamma: with the exact fallback %.2e (dead) %.2e (others); without %.2e (dead)'
          % (tiny, float(err[dead].max()), float(err.max()), float(err_raw[dead].max())))
    assert float(err[dead].max()) <= 2e-3 and float(err.max()) <= 1e-2
    if not helpers_f16() or tiny <= 1e-4:
        assert float(err_raw[dead].max()) > 10 * float(err[dead].max())           # the failure mode the fallback exists for


def test_native_trunk_matches_module_walk():
    """evk_trunk_forward / evk_trunk_backward (one C call per direction) against the op-by-op walk over the same parameter
    holders (conv2d / batchnorm / max-pool autograd wrappers).  Eval mode (running statistics) must agree tightly; in
    train mode the runner takes the batch statistics from the f32 conv accumulators while the walk reduces the bf16-rounded
    output, and the random-weight trunk amplifies that 2^-9 difference (DESIGN.md "Parity"), so only a loose bound holds."""
    import copy
    from evoke_amd import ops, trunk as T

    def rel(x, y):
        return float((x - y).norm() / (y.norm() + 1e-30))

    def walk(b, img):
        x = T._Stem.apply(img, b[0].weight)
        x = b[1](x, relu=True)
        x = T._MaxPool.apply(x)
        for li in range(4, 8):
            for blk in b[li]:
                x = blk(x)
        return x

    torch.manual_seed(11)
    ops.clear_grad_callbacks()
    a = T.ResNetTrunk().cuda()
    with torch.no_grad():
        for m in a.modules():
            if isinstance(m, T.Bottleneck):
                m.bn3.weight.mul_(0.2)
    img = torch.randn(4, 3, 96, 96, device='cuda')
    dout = (torch.randn(4, 3, 3, 2048, device='cuda') * 0.1).to(BF)
    for train, out_tol, grad_tol in ((False, 5e-3, 5e-2), (True, 0.15, None)):
        a.train(train)
        b = copy.deepcopy(a)
        for p in list(a.parameters()) + list(b.parameters()):
            p.grad = None
        ya = a(img)
        ya.backward(dout)
        yb = walk(b, img)
        yb.backward(dout)
        ops.join_side_streams()
        torch.cuda.synchronize()
        e_out = rel(ya.float(), yb.float())
        assert e_out < out_tol, (train, e_out)
        worst = 0.0
        for (na, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
            e = rel(pa.grad.float(), pb.grad.float())
            worst = max(worst, e)
            assert grad_tol is None or e < grad_tol, (train, na, e)
        for (na, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
            assert rel(ba.float(), bb.float()) < (0.15 if train else 1e-6), (train, na)
        print('   native trunk vs module walk (train=%s): out %.3g, worst grad %.3g' % (train, e_out, worst))


AUDIT_CASES = {
    # blocks, planes, N, H, W, ill-conditioned batch-norm parameters.  96 x 160 images: no M is a multiple of a tile (layer4 has 3 x 5 pixels per
    # image), N in {1, 3, 5}; (2,1,2,1) gives layers with a following block behind the strided / shortcut one; the narrow trunk makes a channel
    # group of 8 a whole block of the batch-norm kernels
    'b1111_p64_n5': ((1, 1, 1, 1), (64, 128, 256, 512), 5, 96, 160, False),
    'b2121_p64_n3': ((2, 1, 2, 1), (64, 128, 256, 512), 3, 96, 160, False),
    'b2121_p16_n1': ((2, 1, 2, 1), (16, 32, 64, 128), 1, 96, 160, False),
    'b2121_p64_n3_ill': ((2, 1, 2, 1), (64, 128, 256, 512), 3, 64, 96, True),
    # the full depth: 23 blocks of layer3 behind one another (the skip-chain budget), 104 pairs
    'resnet101_n3_224': ((3, 4, 23, 3), (64, 128, 256, 512), 3, 224, 224, False),
    'resnet101_n2_384': ((3, 4, 23, 3), (64, 128, 256, 512), 2, 384, 384, False),
}
NAN_FILL = 0x7FC0          # a quiet NaN as a 16-bit lane of either storage format, and (0x7FC07FC0) as an f32 lane


def _same_bits(a, b, what):
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if x is None and y is None:
            continue
        if not torch.equal(x.contiguous().view(-1).view(torch.uint8), y.contiguous().view(-1).view(torch.uint8)):
            bad.append(k)
    assert not bad, '%s: not bit-identical: %s' % (what, bad[:12])


def _run_bits(TA, case, res, training=True):
    """everything a run produced, keyed by name, for bit comparisons"""
    out = dict(TA.stored_tensors(case.workspace(res['ws']), training=training))
    out['out'] = res['out']
    for i, g in enumerate(res['grads']):
        for k, v in g.items():
            out['pair%d.%s' % (i, k)] = v
    for i, (a, b) in enumerate(res['running']):
        out['pair%d.running_mean' % i], out['pair%d.running_var' % i] = a, b
    return out


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('name', list(AUDIT_CASES))
def test_native_trunk_matches_module_walk_hop_by_hop_in_fp64(name, training):
    """evk_trunk_forward + evk_trunk_backward through ctypes on a workspace this test owns, audited hop by hop against float64
    (tests/trunk_audit.py: every pair's y, statistics, z, dy, backward sums, parameter-gradient increments from non-zero starts, the stem's
    packing, the max-pool and its recorded taps), with bounds derived from the number formats -- a few units of 16-bit round-off per hop,
    not the 15 % / unbounded-gradient comparison of the end-to-end test above.  Workspace hygiene on the way: the workspace sits between two
    1 MiB guard bands that must come back untouched, and a zero-filled and a NaN-filled workspace must give the same bits everywhere (a
    difference means a kernel read workspace it never wrote); so must the backward with and without a separate weight-gradient stream (the
    trunk's reductions are two-stage, no atomics), and freezing some parameters must not move the others."""
    from evoke_amd import hip as H
    from tests import trunk_audit as TA
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    blocks, planes, N, Hh, Ww, ill = AUDIT_CASES[name]
    case = TA.TrunkCase(blocks, planes, N, Hh, Ww, seed=len(name) + 7 * N, ill=ill)
    if sum(blocks) > 8 and not training:
        case.calibrate()
    zero = case.run(training, 0, side_stream=True)
    nan = case.run(training, NAN_FILL, side_stream=True)
    one = case.run(training, NAN_FILL, side_stream=False)
    for r, what in ((zero, 'zero fill'), (nan, 'NaN fill'), (one, 'NaN fill, one stream')):
        assert r['guards_ok'], '%s: a guard band next to the workspace was written' % what
    _same_bits(_run_bits(TA, case, zero, training), _run_bits(TA, case, nan, training), 'zero-filled against NaN-filled workspace')
    _same_bits(_run_bits(TA, case, nan, training), _run_bits(TA, case, one, training), 'weight gradients on a second stream against one stream')
    # frozen parameters: NULL gradient pointers on some pairs leave every other result unchanged bit for bit
    npairs = len(case.pairs)
    frozen = {(i, k) for i in range(0, npairs, 3) for k in ('dw',)} | {(i, k) for i in range(1, npairs, 4) for k in ('dgamma', 'dbeta')} | {(2, 'dw'), (2, 'dgamma'), (2, 'dbeta')}
    part = case.run(training, NAN_FILL, side_stream=True, frozen=frozen)
    assert part['guards_ok']
    _same_bits({k: v for k, v in _run_bits(TA, case, part, training).items() if v is not None}, _run_bits(TA, case, nan, training), 'partially frozen against fully trainable')
    fails, lines, _ = TA.evaluate(case.audit(nan, training))
    print('   trunk audit %s (%s, %s storage): worst error / bound per pair' % (name, 'train' if training else 'eval', H.STORE))
    print('\n'.join(lines))
    assert not fails, '%d quantities outside their bounds:\n%s' % (len(fails), '\n'.join(fails[:30]))


def test_resnet101_at_the_bench_geometry_hop_by_hop_in_fp64():
    """The same audit at the benchmark's geometry -- resnet101, 64 images of 384 x 384, train mode -- where the host-side routing picks the
    kernels the benchmark runs (it depends on M: halo-tile 3x3 forward / data / weight gradients, strip GEMM, weight-stationary pointwise
    kernels with fused statistics, the halo stem, the folded second reduction stage), which the reduced cases do not all reach.  Default
    build's pass only (the name keeps it out of the bf16 child and of the fallback-route child).  The 20 GB workspace is audited where it is:
    float64 on the device, restricted to matmuls, slices, elementwise operations and reductions (tests/trunk_audit.py: conv_mm; data and
    weight gradients by autograd over it) -- never the library under test, never a vendor convolution.  That device-side reference is first
    validated against the CPU float64 restatement on a reduced case: the two must agree to a 10^-6 of each bound."""
    from evoke_amd import hip as H
    from tests import trunk_audit as TA
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    small = TA.TrunkCase((2, 1, 2, 1), (64, 128, 256, 512), 3, 96, 160, seed=41)
    res = small.run(True, NAN_FILL)
    res_dev = dict(res, ws=res['ws'].cuda())
    n = 0
    for a, b in zip(small.audit(res, True), small.audit(res_dev, True)):
        assert (a.pair, a.name) == (b.pair, b.name)
        wa, wb, ba, bb = a.want.double(), b.want.double().cpu(), a.bound.double(), b.bound.double().cpu()
        assert bool(((wa - wb).abs() <= 1e-6 * ba + 1e-13 * wa.abs()).all()), ('device reference differs from the CPU restatement', a.pair, a.name)
        assert bool(((ba - bb).abs() <= 1e-6 * ba).all()), ('device bound differs from the CPU restatement', a.pair, a.name)
        n += 1
    assert n > 20 * 12
    del res, res_dev, small
    case = TA.TrunkCase((3, 4, 23, 3), (64, 128, 256, 512), 64, 384, 384, seed=64)
    res = case.run(True, NAN_FILL, on_device=True)
    assert res['guards_ok'], 'a guard band next to the workspace was written'
    fails, lines, _ = TA.evaluate(case.audit(res, True))
    print('   trunk audit resnet101 64 x 384 x 384 (train, %s storage): worst error / bound per pair' % H.STORE)
    print('\n'.join(lines))
    assert not fails, '%d quantities outside their bounds:\n%s' % (len(fails), '\n'.join(fails[:30]))


def test_native_trunk_matches_module_walk_on_a_leased_poisoned_workspace():
    """The product path (ResNetTrunk -> _TrunkFn -> the _WsLease pool) on a pool buffer this test seeded: NaN-filled, between guard bands.  Its
    output, parameter gradients and running statistics equal, bit for bit, those of the ctypes calls on a zero-filled workspace of the test's
    own; the guard bands come back untouched."""
    import ctypes as C
    from evoke_amd import hip as H
    from evoke_amd import ops, trunk as T
    from tests import trunk_audit as TA
    torch.manual_seed(5)
    ops.clear_grad_callbacks()
    net = T.ResNetTrunk().cuda().train()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, T.Bottleneck):
                m.bn3.weight.mul_(0.2)
    N, Hh, Ww = 2, 64, 96
    img = torch.randn(N, 3, Hh, Ww, device='cuda')
    dout = (torch.randn(N, Hh // 32, Ww // 32, 2048, device='cuda') * 0.1).to(BF)
    cfg = net.native_cfg()
    nb = H.lib.evk_trunk_ws_bytes(C.byref(cfg), N, Hh, Ww)
    assert nb > 0
    pairs = net.pairs()
    running0 = [(bn.running_mean.clone(), bn.running_var.clone()) for _, bn in pairs]

    def guarded(fill):
        big = torch.full((2 * TA.GUARD + nb,), TA.GUARD_BYTE, dtype=torch.uint8, device='cuda')
        assert big.data_ptr() % 256 == 0
        big[TA.GUARD:TA.GUARD + nb].view(torch.int16).fill_(fill)
        return big

    def guards_ok(big):
        return bool((big[:TA.GUARD] == TA.GUARD_BYTE).all()) and bool((big[TA.GUARD + nb:] == TA.GUARD_BYTE).all())

    big = guarded(NAN_FILL)
    key = (torch.cuda.current_device(), int(nb))
    saved_pool = T._WsLease._pool.pop(key, None)
    T._WsLease._pool[key] = [big[TA.GUARD:TA.GUARD + nb]]
    try:
        out = net(img)
        out.backward(dout)
        ops.join_side_streams()
        torch.cuda.synchronize()
        leased = T._WsLease._pool.get(key) or []
        assert not leased or leased[0].data_ptr() == big.data_ptr() + TA.GUARD          # the seeded buffer was the one used and came back
    finally:
        T._WsLease._pool.pop(key, None)
        if saved_pool is not None:
            T._WsLease._pool[key] = saved_pool
    assert guards_ok(big)
    got = {'out': out.detach().clone()}
    for i, (cv, bn) in enumerate(pairs):
        got['pair%d.dw' % i], got['pair%d.dgamma' % i], got['pair%d.dbeta' % i] = cv.weight.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()
        got['pair%d.running_mean' % i], got['pair%d.running_var' % i] = bn.running_mean.clone(), bn.running_var.clone()
    ws_product = big[TA.GUARD:TA.GUARD + nb].cpu()
    # the same step through ctypes: gradients and running statistics back to their starting values, a zero-filled workspace
    with torch.no_grad():
        for (cv, bn), (rm, rv) in zip(pairs, running0):
            cv.weight.grad.zero_(); bn.weight.grad.zero_(); bn.bias.grad.zero_()
            bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    arr, keep = T._TrunkFn._layers(pairs, True)
    big2 = guarded(0)
    ws2 = big2[TA.GUARD:TA.GUARD + nb]
    out2 = torch.empty_like(out)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    H.check(H.lib.evk_trunk_forward(C.byref(cfg), arr, len(pairs), H.ptr(img), N, Hh, Ww, H.ptr(ws2), nb, H.ptr(out2), 1, H.stream()), 'trunk_forward')
    H.check(H.lib.evk_trunk_backward(C.byref(cfg), arr, len(pairs), N, Hh, Ww, H.ptr(ws2), nb, H.ptr(dout), 1, H.stream(), side.cuda_stream), 'trunk_backward')
    side.synchronize()
    torch.cuda.synchronize()
    assert guards_ok(big2)
    want = {'out': out2}
    for i, (cv, bn) in enumerate(pairs):
        want['pair%d.dw' % i], want['pair%d.dgamma' % i], want['pair%d.dbeta' % i] = cv.weight.grad, bn.weight.grad, bn.bias.grad
        want['pair%d.running_mean' % i], want['pair%d.running_var' % i] = bn.running_mean, bn.running_var
    _same_bits({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()}, 'product path against ctypes run')
    # and everything the runner keeps in the workspace
    pv, plan = H.trunk_plan(cfg, N, Hh, Ww)
    a, b = TA.Workspace(ws_product, pv, plan, H.STORE_DTYPE), TA.Workspace(ws2.cpu(), pv, plan, H.STORE_DTYPE)
    _same_bits(TA.stored_tensors(a), TA.stored_tensors(b), 'leased NaN-filled workspace against zero-filled workspace')


def test_decode_attention_matches_reference():
    """evk_decode_attention (one query per row, whole K/V cache, key mask) against fp32 torch on the same bf16 inputs."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(5)
    for (R, S, heads, masked) in [(7, 100, 8, True), (256, 144, 8, False), (3, 1, 8, True), (5, 256, 4, True)]:
        HD = heads * 64
        q = (torch.randn(R, 1, HD, device='cuda') * 0.8).to(BF)
        k = (torch.randn(R, S, HD, device='cuda') * 0.8).to(BF)
        v = torch.randn(R, S, HD, device='cuda').to(BF)
        mask = None
        if masked:
            lens = torch.randint(1, S + 1, (R,), device='cuda')
            mask = (torch.arange(S, device='cuda').unsqueeze(0) < lens.unsqueeze(1)).to(torch.uint8).contiguous()
        out = torch.empty_like(q)
        H.check(H.lib.evk_decode_attention(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask) if mask is not None else None, H.ptr(out), R, S,
                                           heads, 64, 1, C.c_float(0.125), H.stream()))
        qf = q.float().view(R, heads, 1, 64)
        kf = k.float().view(R, S, heads, 64).permute(0, 2, 1, 3)
        vf = v.float().view(R, S, heads, 64).permute(0, 2, 1, 3)
        sc = (qf @ kf.transpose(-1, -2)) * 0.125
        if mask is not None:
            sc = sc.masked_fill(mask.view(R, 1, 1, S) == 0, float('-inf'))
        ref_o = (torch.softmax(sc, -1) @ vf).permute(0, 2, 1, 3).reshape(R, 1, HD)
        close(out.float(), ref_o.cpu(), 1e-2, 1e-2, 'decode attention R=%d S=%d' % (R, S))
        if R % 4 == 0:          # beams of a sample sharing one K / V / mask row
            q4 = q.repeat_interleave(4, 0).contiguous()
            q4 = (q4 + torch.randn_like(q4.float()).to(BF) * 0.1).contiguous()
            out4 = torch.empty_like(q4)
            H.check(H.lib.evk_decode_attention(H.ptr(q4), H.ptr(k), H.ptr(v), H.ptr(mask) if mask is not None else None, H.ptr(out4), 4 * R, S,
                                               heads, 64, 4, C.c_float(0.125), H.stream()))
            k4, v4 = k.repeat_interleave(4, 0).contiguous(), v.repeat_interleave(4, 0).contiguous()
            m4 = mask.repeat_interleave(4, 0).contiguous() if mask is not None else None
            ref4 = torch.empty_like(q4)
            H.check(H.lib.evk_decode_attention(H.ptr(q4), H.ptr(k4), H.ptr(v4), H.ptr(m4) if m4 is not None else None, H.ptr(ref4), 4 * R, S,
                                               heads, 64, 1, C.c_float(0.125), H.stream()))
            assert torch.equal(out4, ref4)
        # cache indirection: position s of hypothesis r lives in cache row rowmap[r, s] -> same bits as gathering the caches
        rowmap = torch.randint(0, R, (R, S), device='cuda', dtype=torch.int32)
        gi = rowmap.long().unsqueeze(-1).expand(R, S, HD)
        kg, vg = k.gather(0, gi).contiguous(), v.gather(0, gi).contiguous()
        ref_i, out_i = torch.empty_like(q), torch.empty_like(q)
        H.check(H.lib.evk_decode_attention(H.ptr(q), H.ptr(kg), H.ptr(vg), H.ptr(mask) if mask is not None else None, H.ptr(ref_i), R, S,
                                           heads, 64, 1, C.c_float(0.125), H.stream()))
        H.check(H.lib.evk_decode_attention_indirect(H.ptr(q), H.ptr(k), H.ptr(v), H.ptr(mask) if mask is not None else None, H.ptr(rowmap),
                                                    None, H.ptr(out_i), R, S, heads, 64, C.c_float(0.125), H.stream()))
        assert torch.equal(out_i, ref_i)
        # device-side step index instead of a mask: positions > last_pos are neither read nor attended
        lp = torch.tensor([S // 2], device='cuda', dtype=torch.long)
        causal = (torch.arange(S, device='cuda') <= lp).to(torch.uint8).unsqueeze(0).expand(R, S).contiguous()
        H.check(H.lib.evk_decode_attention(H.ptr(q), H.ptr(kg), H.ptr(vg), H.ptr(causal), H.ptr(ref_i), R, S, heads, 64, 1, C.c_float(0.125),
                                           H.stream()))
        H.check(H.lib.evk_decode_attention_indirect(H.ptr(q), H.ptr(k), H.ptr(v), None, H.ptr(rowmap), H.ptr(lp), H.ptr(out_i), R, S, heads, 64,
                                                    C.c_float(0.125), H.stream()))
        assert torch.equal(out_i, ref_i)


def test_native_trunk_frozen_parameters_and_no_grad():
    """Partially frozen trunk (conv weights frozen, batch-norm affine trainable), fully frozen trunk, and no_grad inference."""
    from evoke_amd import ops, trunk as T
    torch.manual_seed(3)
    ops.clear_grad_callbacks()
    t = T.ResNetTrunk().cuda().train()
    img = torch.randn(2, 3, 64, 64, device='cuda')
    for cv, bn in t.pairs():
        cv.weight.requires_grad_(False)
    y = t(img)
    y.float().square().mean().backward()
    ops.join_side_streams()
    torch.cuda.synchronize()
    for cv, bn in t.pairs():
        assert cv.weight.grad is None
        assert bn.weight.grad is not None and torch.isfinite(bn.weight.grad).all() and torch.isfinite(bn.bias.grad).all()
    assert float(t[7][2].bn3.weight.grad.abs().sum()) > 0
    for p in t.parameters():
        p.requires_grad_(False)
        p.grad = None
    y2 = t(img)
    assert not y2.requires_grad and torch.isfinite(y2.float()).all()
    t.eval()
    with torch.no_grad():
        y3 = t(img)
    assert y3.shape == (2, 2, 2, 2048) and torch.isfinite(y3.float()).all()


@pytest.mark.parametrize('R,N,cond,act,f32', [(256, 1536, True, 0, False), (256, 512, True, 1, False), (256, 1445, False, 0, True), (37, 512, True, 0, False),
                                              (1, 16, False, 0, False)])
def test_linear_with_layernorm_in_the_operand_load_equals_norm_then_linear(R, N, cond, act, f32):
    """evk_linear_ln (the decode step's `x + f(norm(x))` sublayers, encoder_decoder.py:114-126, 144-179, as one launch per projection)
    against the two launches it replaces -- evk_layernorm_fwd (R2Gen mode, optional conditional deltas) then the skinny GEMM.  The
    prologue repeats the norm kernel's arithmetic term for term on the same lane / element mapping, so the result must be BIT-identical
    (beam search compares scores for ties: a last-bit difference could change a token)."""
    import ctypes as C
    from evoke_amd import hip as H, ops
    torch.manual_seed(R + N)
    K = 512
    x = (torch.randn(R, K, device='cuda') * 1.3 + 0.2).to(BF)
    gamma, beta = 1 + 0.1 * torch.randn(K, device='cuda'), 0.1 * torch.randn(K, device='cuda')
    dg = (0.05 * torch.randn(R, K, device='cuda')).to(BF) if cond else None
    db = (0.05 * torch.randn(R, K, device='cuda')).to(BF) if cond else None
    Np = (N + 7) // 8 * 8
    w = torch.zeros(Np, K, device='cuda', dtype=BF)
    w[:N] = (torch.randn(N, K, device='cuda') * 0.05).to(BF)
    bias = 0.1 * torch.randn(N, device='cuda')
    resid = (torch.randn(R, Np, device='cuda') * 0.5).to(BF) if act == 0 and not f32 else None
    odt = torch.float32 if f32 else BF
    with torch.no_grad():
        n = ops.layernorm(x, gamma, beta, eps=1e-6, mode=1, dgam=dg, dbet=db)
        want = torch.zeros(R, Np, device='cuda', dtype=odt)
        ops.gemm(n, w, want, R, N, K, lda=K, ldb=K, ldc=Np, bias=bias, resid=resid, ldr=Np, act=act)
    got = torch.zeros(R, Np, device='cuda', dtype=odt)
    H.check(H.lib.evk_linear_ln(H.ptr(x), H.ptr(gamma), H.ptr(beta), H.ptr(dg) if cond else None, H.ptr(db) if cond else None, K if cond else 0,
                                C.c_float(1e-6), 1, H.ptr(w), H.ptr(bias), H.ptr(resid) if resid is not None else None, Np, H.ptr(got),
                                H.F32 if f32 else H.BF16, Np, R, N, K, act, H.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want), 'max |d| %.3g' % float((got.float() - want.float()).abs().max())
    # and against fp32 torch on the same operands (R2Gen norm: unbiased std, eps added to the std)
    xf = x.float()
    g, b = gamma + (dg.float() if cond else 0), beta + (db.float() if cond else 0)
    ref = (g * (xf - xf.mean(-1, keepdim=True)) / (xf.std(-1, keepdim=True) + 1e-6) + b) @ w[:N].float().t() + bias
    if act == 1:
        ref = torch.relu(ref)
    if resid is not None:
        ref = ref + resid[:, :N].float()
    close(got[:, :N].float(), ref.cpu(), 2e-2, 2e-2, 'linear_ln vs fp32')


@pytest.mark.parametrize('R,S,pos', [(256, 100, 0), (256, 100, 57), (12, 100, 99), (5, 256, 130)])
def test_decode_attention_fed_by_the_fused_projection_equals_append_then_attend(R, S, pos):
    """evk_decode_attention_qkv (q read in place from the q | k | v projection, this step's key / value attended to and appended by
    the same launch) against the three steps it replaces: slice q, write k / v into cache row r at *last_pos, evk_decode_attention_indirect
    over the row table.  Same arithmetic in the same order: outputs and caches must be BIT-identical (beam search ranks on them).
    The row table sends every earlier position to some other hypothesis' cache row, as after beam re-ordering."""
    import ctypes as C
    from evoke_amd import hip as H
    torch.manual_seed(R + S + pos)
    heads, HD = 8, 512
    qkv = (torch.randn(R, 3 * HD, device='cuda') * 0.7).to(BF)
    ks = (torch.randn(R, S, HD, device='cuda') * 0.7).to(BF)
    vs = torch.randn(R, S, HD, device='cuda').to(BF)
    anc = torch.randint(0, R, (R, S), device='cuda', dtype=torch.int32)
    anc[:, pos] = torch.arange(R, device='cuda', dtype=torch.int32)           # the position being written lives in the hypothesis' own row
    lp = torch.tensor([pos], device='cuda', dtype=torch.long)
    # reference path
    k0, v0 = ks.clone(), vs.clone()
    k0[:, pos] = qkv[:, HD:2 * HD]
    v0[:, pos] = qkv[:, 2 * HD:]
    q = qkv[:, :HD].contiguous().view(R, 1, HD)
    want = torch.empty_like(q)
    H.check(H.lib.evk_decode_attention_indirect(H.ptr(q), H.ptr(k0), H.ptr(v0), None, H.ptr(anc), H.ptr(lp), H.ptr(want), R, S, heads, 64,
                                                C.c_float(0.125), H.stream()))
    # fused path
    k1, v1 = ks.clone(), vs.clone()
    got = torch.empty(R, 1, HD, device='cuda', dtype=BF)
    H.check(H.lib.evk_decode_attention_qkv(H.ptr(qkv), 3 * HD, H.ptr(k1), H.ptr(v1), H.ptr(anc), H.ptr(lp), H.ptr(got), R, S, heads, 64,
                                           C.c_float(0.125), H.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(k1, k0) and torch.equal(v1, v0)
    # and against fp32 torch: positions <= pos, each read from the row the table names
    rows = anc[:, :pos + 1].long()
    kk = k0[rows, torch.arange(pos + 1, device='cuda')].float().view(R, pos + 1, heads, 64).permute(0, 2, 1, 3)
    vv = v0[rows, torch.arange(pos + 1, device='cuda')].float().view(R, pos + 1, heads, 64).permute(0, 2, 1, 3)
    sc = (q.float().view(R, heads, 1, 64) @ kk.transpose(-1, -2)) * 0.125
    ref = (torch.softmax(sc, -1) @ vv).permute(0, 2, 1, 3).reshape(R, 1, HD)
    close(got.float(), ref.cpu(), 1e-2, 1e-2, 'decode attention qkv R=%d S=%d pos=%d' % (R, S, pos))


def test_cu_masked_stream_runs_kernels_on_its_share_of_the_compute_units():
    """evk_stream_create_cu_mask / hip.masked_stream: a stream whose kernels keep off 8, 16 or 24 of every 32 CUs: a kernel
    launched on the stream produces the same bytes as on the default stream, and a bad request is refused."""
    import ctypes as C
    from evoke_amd import hip as H
    n = C.c_int32(0)
    H.check(H.lib.evk_device_cu_count(0, C.byref(n)), 'device_cu_count')
    assert n.value >= 64
    x = rnd(4096, 512).to(BF).cuda()
    want = torch.empty(4096, 512, dtype=torch.float32, device='cuda')
    H.check(H.lib.evk_cast(H.ptr(x), H.BF16, H.ptr(want), H.F32, x.numel(), H.stream()), 'cast')
    torch.cuda.synchronize()
    for reserve in (8, 16, 24):
        st = H.masked_stream('cuda:0', reserve)
        assert H.masked_stream('cuda:0', reserve) is st                      # cached: one stream per (device, share)
        got = torch.empty_like(want)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            H.check(H.lib.evk_cast(H.ptr(x), H.BF16, H.ptr(got), H.F32, x.numel(), H.stream()), 'cast on the masked stream')
        st.synchronize()
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        H.masked_stream('cuda:0', 5)
    out = C.c_void_p()
    assert H.lib.evk_stream_create_cu_mask(None, 0, C.byref(out)) == -1       # EVK_EINVAL


def test_streams_concurrent_tells_shared_hardware_queues_from_separate_ones():
    """evk_streams_concurrent (the check the step replayer runs over its lanes before the first replay): a stream against itself is not
    concurrent; hip.concurrent_streams hands out streams that are pairwise concurrent with each other and with the current stream, and the
    check agrees with a direct timing of two 150 us spin kernels."""
    from evoke_amd import hip as H
    cur = torch.cuda.current_stream()
    assert not H.streams_concurrent(cur, cur)
    a, b = H.concurrent_streams(2, against=[cur])
    assert H.streams_concurrent(a, b) and H.streams_concurrent(cur, a) and H.streams_concurrent(cur, b)
    torch.cuda.synchronize()
