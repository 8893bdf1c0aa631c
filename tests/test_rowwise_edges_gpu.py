"""GPU edge tests of the row-wise and element-wise kernels (csrc/norm.hip, csrc/eltwise.hip) through the C ABI, and of the unfused attention
route (ops._Attention) that is built on them, against the float64 restatements of tests/rowwise_reference.py (pinned to torch by
tests/test_rowwise_reference_cpu.py).  The error model -- where every bound comes from -- is that module's docstring.

Conventions: every output buffer is pre-filled with NaN (123 for integers) and sits between guard bands that must come back untouched;
pad columns of inputs hold NaN, so a kernel that reads them shows it; no index outside a buffer is ever passed.  Every test prints the worst
error it saw as a fraction of its bound."""
import math

import pytest
import torch

from tests import rowwise_reference as R
from tests.helpers import STORE_DTYPE as BF

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN, INF = float('nan'), float('inf')
G = 64                       # guard elements either side of an output
GUARD = 768.0               # exact in both 16-bit formats


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(*shape, seed):
    return torch.randn(*shape, generator=gen(seed))


def pad8(n):
    return (n + 7) // 8 * 8


def dcode(dtype):
    from evoke_amd import hip as H
    return H.F32 if dtype == F32 else H.BF16


class Buf:
    """a device output of n elements, pre-filled, between two guard bands"""

    def __init__(self, n, dtype=F32, fill=NAN):
        self.all = torch.full((n + 2 * G,), GUARD if dtype.is_floating_point else int(GUARD), dtype=dtype, device='cuda')
        self.t = self.all[G:G + n]
        self.t.fill_(fill)

    @classmethod
    def of(cls, values, dtype=None):
        """a guarded buffer that starts from `values` (accumulators)"""
        b = cls(values.numel(), dtype or values.dtype)
        b.t.copy_(values.reshape(-1))
        return b

    @property
    def ptr(self):
        return self.t.data_ptr()

    def cpu(self, *shape):
        g = self.all.cpu()
        assert bool((g[:G] == g[0]).all()) and bool((g[-G:] == g[0]).all()) and float(g[0]) == GUARD, 'a guard band was written'
        out = g[G:-G]
        return out.view(*shape) if shape else out


_LIVE = []


def dptr(t):
    """device pointer of t, uploaded first when it lives on the host.  The device tensor is kept until the end of the test: a temporary
    would be released as soon as its pointer is taken, and the caching allocator hands the block to the NEXT upload of the same call --
    before the kernel has been launched."""
    if t is None:
        return None
    d = t if t.is_cuda else t.cuda()
    _LIVE.append(d)
    return d.data_ptr()


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _LIVE.clear()


def up(t, dtype=None):
    """CPU tensor -> device (rounded to dtype); the rounded values come back as the second result, for the reference"""
    d = t.to(dtype if dtype is not None else t.dtype).contiguous()
    return d.cuda(), d


class Worst:
    """collects |err| / bound; a NaN where a number is expected counts as beyond every bound"""

    def __init__(self, name):
        self.name, self.w, self.u = name, 0.0, 0.0

    def __call__(self, what, got, want, tol, ulps=False):
        """ulps: also record the worst |err| in units of the storage format's ulp alone (what the bound would have to be without its f32 term)"""
        got, want = got.detach().to(F64).cpu(), want.detach().to(F64).cpu()
        tol = torch.as_tensor(tol, dtype=F64).expand_as(want)
        err = (got - want).abs()
        both_inf = torch.isinf(want) & (got == want)
        err = torch.where(both_inf, torch.zeros_like(err), err)
        ok = err <= tol
        if err.numel():
            ratio = torch.where(tol > 0, err / tol, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
            ratio = torch.nan_to_num(ratio, nan=INF)
            i = int(ratio.argmax())
            assert bool(ok.all()), '%s %s: %d of %d beyond the bound; worst: got %r want %r (bound %.4g) at flat index %d' % (
                self.name, what, int((~ok).sum()), ok.numel(), float(got.reshape(-1)[i]), float(want.reshape(-1)[i]), float(tol.reshape(-1)[i]), i)
            self.w = max(self.w, float(ratio.max()))
            if ulps:
                self.u = max(self.u, float(torch.nan_to_num(err / R.ulp(want, BF), nan=INF).max()))

    def done(self, note=''):
        print('%s: worst |err| / bound = %.3f %s%s' % (self.name, self.w, note, '; 16-bit outputs with an f32 term: worst |err| = %.1f ulp' % self.u if self.u else ''))


EPS = 2.0 ** -24                # unit roundoff of f32


def tol16(want, f32_term=None):
    """one unit in the last place of the storage format at the float64 value.  f32_term: for outputs whose f32 arithmetic subtracts nearly equal
    quantities, the f32 rounding error of that arithmetic, a few EPS times the MAGNITUDES OF THE OPERANDS taken from the float64 reference --
    it is far below one ulp wherever nothing cancels, and each caller derives its own"""
    t = R.ulp(want, BF)
    return t if f32_term is None else t + f32_term


# =============================================================================================================== A. unfused attention route
def _attention_inputs(cfg):
    B, T, S, Hh, dh = cfg['B'], cfg['T'], cfg['S'], cfg['Hh'], cfg['dh']
    q, k, v, do = randn(B, T, Hh * dh, seed=1), randn(B, S, Hh * dh, seed=2), randn(B, S, Hh * dh, seed=3), randn(B, T, Hh * dh, seed=4)
    mask = None
    if cfg['mask'] == 'full':
        mask = (torch.rand(B, T, S, generator=gen(9)) > 0.3).to(torch.uint8)
        mask[:, :, 0] = 1
    elif cfg['mask']:
        mask = torch.ones(B, S, dtype=torch.uint8)
        for i in range(B):
            mask[i, S - 3 * i:] = 0
    return q, k, v, do, mask


def _attention_ref(cfg, q, k, v, do, mask):
    """the reference of tests/test_hip_ops.py::test_attention on the 16-bit-rounded inputs, in float64"""
    B, T, S, Hh, dh = cfg['B'], cfg['T'], cfg['S'], cfg['Hh'], cfg['dh']
    qr, kr, vr = (t.to(BF).to(F64).requires_grad_(True) for t in (q, k, v))
    sc = torch.einsum('bthd,bshd->bhts', qr.view(B, T, Hh, dh), kr.view(B, S, Hh, dh)) / math.sqrt(dh)
    if mask is not None:
        sc = sc.masked_fill((mask[:, None, :, :] if mask.dim() == 3 else mask[:, None, None, :]) == 0, -1e9)
    if cfg['mask'] == 'causal':
        sc = sc.masked_fill(torch.tril(torch.ones(T, S)) == 0, -1e9)
    orf = torch.einsum('bhts,bshd->bthd', torch.softmax(sc, -1), vr.view(B, S, Hh, dh)).reshape(B, T, Hh * dh)
    orf.backward(do.to(BF).to(F64))
    return orf.detach(), qr.grad, kr.grad, vr.grad


ATT_BOUNDS = (('o', 2e-2), ('dq', 3e-2), ('dk', 3e-2), ('dv', 3e-2))            # rtol == atol, the bounds of test_attention


def _attention_check(w, what, got, want, scale=1.0):
    for (name, b), g_, w_ in zip(ATT_BOUNDS, got, want):
        w('%s %s' % (what, name), g_, w_, scale * (b + b * w_.to(F64).abs().cpu()))


def _run_attention(fn, cfg, q, k, v, do, mask):
    qd, kd, vd = (t.to(BF).cuda().requires_grad_(True) for t in (q, k, v))
    o = fn(qd, kd, vd, mask.cuda() if mask is not None else None)
    o.backward(do.to(BF).cuda())
    torch.cuda.synchronize()
    return o.detach(), qd.grad, kd.grad, vd.grad


@pytest.mark.parametrize('cfg', [dict(B=2, T=37, S=650, Hh=4, dh=64, mask='key'), dict(B=1, T=33, S=1024, Hh=2, dh=64, mask='full'),
                                 dict(B=1, T=700, S=700, Hh=2, dh=64, mask='causal'), dict(B=2, T=40, S=50, Hh=4, dh=96, mask=None)],
                         ids=lambda c: 'S%d_dh%d_%s' % (c['S'], c['dh'], c['mask']))
def test_unfused_attention_route_taken_by_long_rows_and_odd_heads(cfg):
    """ops.attention where evk_attention_supported(S, dh) is 0 -- padded S above 640, or dh no multiple of 64 --, i.e. ops._Attention:
    batched score GEMM, evk_softmax_fwd / _bwd on 16-bit probabilities with key, full and causal masks, P.V with K = pad8(S).  (The zeroed pad columns of P are pinned by the
    softmax test below, not here: this route also zero-pads V.)  Forward and backward against float64 on the rounded inputs, at test_attention's bounds."""
    from evoke_amd import hip as H, ops
    assert H.lib.evk_attention_supported(cfg['S'], cfg['dh']) == 0
    q, k, v, do, mask = _attention_inputs(cfg)
    got = _run_attention(lambda a, b, c, m: ops.attention(a, b, c, cfg['Hh'], mask=m, causal=cfg['mask'] == 'causal'), cfg, q, k, v, do, mask)
    w = Worst('unfused attention %s' % cfg)
    _attention_check(w, 'route', got, _attention_ref(cfg, q, k, v, do, mask))
    w.done()


@pytest.mark.parametrize('cfg', [dict(B=3, T=37, S=50, Hh=12, dh=64, mask='key'), dict(B=3, T=33, S=70, Hh=4, dh=64, mask='full')],
                         ids=lambda c: 'S%d_%s' % (c['S'], c['mask']))
def test_unfused_attention_agrees_with_the_fused_route_where_both_apply(cfg):
    """two configurations of test_attention through ops._Attention.apply directly: against float64 at test_attention's bounds, and against
    the fused route's result within the sum of both bounds"""
    from evoke_amd import hip as H, ops
    assert H.lib.evk_attention_supported(cfg['S'], cfg['dh']) == 1
    q, k, v, do, mask = _attention_inputs(cfg)
    scale = 1.0 / math.sqrt(cfg['dh'])
    unf = _run_attention(lambda a, b, c, m: ops._Attention.apply(a, b, c, m, cfg['Hh'], scale, False, 0.0, 0), cfg, q, k, v, do, mask)
    fus = _run_attention(lambda a, b, c, m: ops._FusedAttention.apply(a, b, c, m, cfg['Hh'], scale, False, 0.0, 0), cfg, q, k, v, do, mask)
    want = _attention_ref(cfg, q, k, v, do, mask)
    w = Worst('unfused vs fused attention %s' % cfg)
    _attention_check(w, 'unfused', unf, want)
    _attention_check(w, 'fused', fus, want)
    _attention_check(w, 'unfused - fused', unf, [f.to(F64).cpu() for f in fus], scale=2.0)
    w.done()


def test_unfused_attention_refuses_rows_longer_than_the_softmax_kernel_holds():
    """S = 1025 (padded 1032 > 64 lanes x 16 columns) must raise from softmax_fwd, not return a result"""
    from evoke_amd import hip as H, ops
    assert H.lib.evk_attention_supported(1025, 64) == 0
    q, k = torch.zeros(1, 4, 128, dtype=BF, device='cuda'), torch.zeros(1, 1025, 128, dtype=BF, device='cuda')
    with pytest.raises(RuntimeError, match='softmax_fwd'):
        ops.attention(q, k, k.clone(), 2)


# =============================================================================================================== B. softmax kernels
SM_S = [1, 63, 64, 65, 435, 1024]
SM_MASKS = ['none', 'key', 'full', 'causal', 'key+causal']
SM_SCORES = ['randn', 'wide', 'offset', 'ninf']


def _sm_masks(kind, B, Tq, S, seed):
    """(mask tensor or None, batch stride, query stride, causal)"""
    if kind in ('none', 'causal'):
        return None, 0, 0, kind == 'causal'
    if kind == 'full':
        m = (torch.rand(B, Tq, S, generator=gen(seed)) > 0.3).to(torch.uint8)
        m[1, 2] = 0                                   # a query without any key
        return m, Tq * S, S, False
    m = (torch.rand(B, S, generator=gen(seed)) > 0.3).to(torch.uint8)
    m[0, 0], m[1, 0] = 1, 0                           # with causal: query 0 of batch 1 has no key at all
    return m, S, 0, kind == 'key+causal'


def _sm_scores(kind, B, heads, Tq, S, ld_in, seed):
    s = randn(B, heads, Tq, S, seed=seed)
    if kind == 'wide':
        s = s * 30                                    # most of a row underflows
    elif kind == 'offset':
        s = s + 3e4
    elif kind == 'ninf':
        s = s.masked_fill(torch.rand(B, heads, Tq, S, generator=gen(seed + 1)) < 0.3, -INF)
        s[0, 0, 1] = -INF                             # a row of -inf only
    full = torch.full((B, heads, Tq, ld_in), NAN)
    full[..., :S] = s
    return full, s


def test_softmax_forward_masks_pads_and_extreme_scores():
    """evk_softmax_fwd: P against the float64 masked softmax for S around the 64-lane and the 16-column limits, padded and unpadded score
    rows, both output strides, 1 and 3 heads (the mask index zo = row / Tq / heads), f32 and 16-bit P, every mask kind, and scores that
    underflow, sit at +3e4 or are -inf.  Columns [S, ld_out) are exactly 0; a row without keys is exactly 0, never NaN."""
    from evoke_amd import hip as H
    B, Tq = 2, 7
    w = Worst('softmax_fwd')
    i = 0
    seen = set()
    for si, S in enumerate(SM_S):
        for mi, mk in enumerate(SM_MASKS):
            for pi, p_dtype in enumerate((F32, BF)):
                i += 1
                # the other axes rotate with (S, mask) and are shifted by one for the second dtype, so that over the six S every mask kind meets
                # both head counts, both strides and every score kind IN BOTH DTYPES (checked after the loop)
                j = si + mi + pi
                heads = (1, 3)[j % 2]
                ld_in = S if (si + pi) % 2 else S + 5
                ld_out = pad8(S) if (si // 2 + mi + pi) % 2 else 1024
                sk = SM_SCORES[(si + 2 * mi + pi) % 4]
                seen |= {(mk, p_dtype, 'heads', heads), (mk, p_dtype, 'ld_in', ld_in == S), (mk, p_dtype, 'ld_out', ld_out == 1024), (mk, p_dtype, sk)}
                mask, mb, mq, causal = _sm_masks(mk, B, Tq, S, seed=i)
                full, s = _sm_scores(sk, B, heads, Tq, S, ld_in, seed=100 + i)
                out = Buf(B * heads * Tq * ld_out, p_dtype)
                H.check(H.lib.evk_softmax_fwd(dptr(full), out.ptr, None, dcode(p_dtype), dptr(mask),
                                              mb, mq, int(causal), B, heads, Tq, S, ld_in, ld_out, 0.0, 0, H.stream()), 'softmax_fwd')
                got = out.cpu(B, heads, Tq, ld_out)
                on = R.attend(B, heads, Tq, S, mask, causal)
                want = R.masked_softmax(s, on)
                what = 'S=%d %s %s %s heads=%d ld_in=%d ld_out=%d' % (S, mk, sk, p_dtype, heads, ld_in, ld_out)
                extra = 4 * R.spacing_f32(3e4 + 6) if sk == 'offset' and p_dtype == F32 else 0.0
                w(what, got[..., :S], want, R.f32_tol(want, extra) if p_dtype == F32 else tol16(want))
                assert bool((got[..., S:] == 0).all()), what + ': pad columns of P are not zero'
                dead = ~(on & torch.isfinite(s)).any(-1)
                assert bool((got[dead] == 0).all()), what + ': a row without keys is not exactly zero'
    assert len(seen) == len(SM_MASKS) * 2 * (2 + 2 + 2 + 4), 'a cell of the grid is not covered'
    w.done('(f32: 1e-5 + 1e-5 |P|; 16-bit: 1 ulp)')


def test_softmax_backward_exact_on_dyadic_data_and_close_on_real_probabilities():
    """evk_softmax_bwd, dS = alpha P (dP - sum dP P): with P in sixteenths, dP in halves and alpha = 1/8 every f32 operation is exact, so
    dS must EQUAL the float64 result rounded once (f32 and 16-bit P, f32 and 16-bit dP, ld_dp != ld); with real probabilities the f32
    bound, for 16-bit dS one ulp (measured 0.5: no element of these rows cancels far enough to need more).  Pad columns of dS are 0, a zero row of P gives a zero row of dS."""
    from evoke_amd import hip as H
    rows = 11
    w = Worst('softmax_bwd')
    i = 0
    for S in SM_S:
        for p_dtype in (F32, BF):
            for dp_dtype in (F32, BF):
                for real in (False, True):
                    i += 1
                    ld = pad8(S) if i % 2 else 1024
                    ld_dp = S + 3 if i % 3 else ld + 8
                    if real:
                        P = torch.softmax(randn(rows, S, seed=i) * 2, -1)
                        dP, alpha = randn(rows, S, seed=i + 1), 0.3
                    else:
                        P = torch.randint(0, 17, (rows, S), generator=gen(i)).float() / 16
                        dP, alpha = torch.randint(-8, 9, (rows, S), generator=gen(i + 1)).float() / 2, 0.125
                    P[1] = 0
                    Pf, dPf = torch.full((rows, ld), NAN), torch.full((rows, ld_dp), NAN)
                    Pf[:, :S], dPf[:, :S] = P, dP
                    Pd, Pr = up(Pf, p_dtype)
                    dPd, dPr = up(dPf, dp_dtype)
                    out = Buf(rows * ld, p_dtype)
                    H.check(H.lib.evk_softmax_bwd(dptr(dPd), dcode(dp_dtype), ld_dp, dptr(Pd), out.ptr, dcode(p_dtype), rows, S, ld, alpha,
                                                  0.0, 0, H.stream()), 'softmax_bwd')
                    got = out.cpu(rows, ld)
                    want = R.softmax_bwd(Pr[:, :S], dPr[:, :S], alpha)
                    what = 'S=%d P %s dP %s ld=%d ld_dp=%d %s' % (S, p_dtype, dp_dtype, ld, ld_dp, 'real' if real else 'dyadic')
                    if real:
                        w(what, got[:, :S], want, R.f32_tol(want) if p_dtype == F32 else tol16(want))
                    else:
                        assert float(alpha * 16 * 32) == 64.0
                        assert bool((got[:, :S].to(F64) == want.to(F32).to(p_dtype).to(F64)).all()), what + ': not the exact result rounded once'
                    assert bool((got[:, S:] == 0).all()), what + ': pad columns of dS are not zero'
                    assert bool((got[1] == 0).all()), what + ': a zero row of P must give a zero row of dS'
    w.done('(real data; f32: 1e-5 + 1e-5 |dS|, 16-bit: 1 ulp; dyadic data: exact)')


def test_softmax_dropout_forward_and_backward_draw_the_same_mask():
    """p = 0.25 on 600 rows of S = 70 (pad8 72, so an index built with S instead of the row stride differs): the keep mask is P' != 0;
    P' = P / (1 - p) under it within one storage rounding; the kept share is 0.75 +- 0.02 over 42000 entries (4 sigma = 0.009);
    evk_softmax_bwd with the same seed gives the float64 dS computed with THAT mask (bound: the f32 bound; in 16 bits one ulp);
    another seed gives another mask."""
    from evoke_amd import hip as H
    B, heads, Tq, S, Sp, p, seed, alpha = 2, 3, 100, 70, 72, 0.25, 20240607, 0.125
    rows = B * heads * Tq
    w = Worst('softmax dropout')
    for p_dtype in (BF, F32):
        s = 0.5 * randn(B, heads, Tq, S, seed=5)
        sd = s.cuda()
        P, Pd, P2, Pd2 = (Buf(rows * Sp, p_dtype) for _ in range(4))
        H.check(H.lib.evk_softmax_fwd(dptr(sd), P.ptr, Pd.ptr, dcode(p_dtype), None, 0, 0, 0, B, heads, Tq, S, S, Sp, p, seed, H.stream()))
        H.check(H.lib.evk_softmax_fwd(dptr(sd), P2.ptr, Pd2.ptr, dcode(p_dtype), None, 0, 0, 0, B, heads, Tq, S, S, Sp, p,
                                      seed + 1, H.stream()))
        Pc, Pdc, Pd2c = P.cpu(rows, Sp), Pd.cpu(rows, Sp), Pd2.cpu(rows, Sp)
        want = R.masked_softmax(s, R.attend(B, heads, Tq, S)).view(rows, S)
        assert float(want.min()) > 2.0 ** -14 * 16, 'every probability must sit far above the 16-bit underflow'
        keep = Pdc[:, :S] != 0
        share = float(keep.double().mean())
        assert keep.numel() >= 40000 and abs(share - (1 - p)) <= 0.02, share
        w('P %s' % p_dtype, Pc[:, :S], want, R.f32_tol(want) if p_dtype == F32 else tol16(want))
        wd = want / (1 - p) * keep
        w("P' %s" % p_dtype, Pdc[:, :S], wd, R.f32_tol(wd) if p_dtype == F32 else tol16(wd))
        assert bool((Pdc[:, :S][~keep] == 0).all()) and bool((Pdc[:, S:] == 0).all()) and bool((Pc[:, S:] == 0).all())
        other = Pd2c[:, :S] != 0
        assert float((other != keep).double().mean()) > 0.25, 'another seed must draw another mask'          # independent masks differ in 37.5 %
        # backward: dP f32 with its own stride, the stored pre-dropout P, the same seed
        ld_dp = 80
        dPf = torch.full((rows, ld_dp), NAN)
        dPf[:, :S] = randn(rows, S, seed=6)
        dS = Buf(rows * Sp, p_dtype)
        H.check(H.lib.evk_softmax_bwd(dptr(dPf), H.F32, ld_dp, P.ptr, dS.ptr, dcode(p_dtype), rows, S, Sp, alpha, p, seed, H.stream()))
        got = dS.cpu(rows, Sp)
        wds = R.softmax_bwd(Pc[:, :S], dPf[:, :S].to(F64) * keep / (1 - p), alpha)
        w('dS %s' % p_dtype, got[:, :S], wds, R.f32_tol(wds) if p_dtype == F32 else tol16(wds))
        assert bool((got[:, S:] == 0).all())
        print('kept share %.4f (%s)' % (share, p_dtype))
    w.done()


# =============================================================================================================== C. LayerNorm kernels
LN_ROWS = [1, 3, 4, 5, 2049, 2053]
LN_D = [8, 520, 2040, 2048]


def _ln_params(rows, D, deltas, seed):
    g, b = 1 + 0.2 * randn(D, seed=seed), 0.1 * randn(D, seed=seed + 1)
    dg = 0.3 * randn(rows, D, seed=seed + 2) if deltas else None
    db = 0.3 * randn(rows, D, seed=seed + 3) if deltas else None
    return g, b, dg, db


def _ln_fwd(x_d, x_dtype, y_dtype, g, b, dg_d, db_d, d_dtype, rows, D, mode, eps):
    from evoke_amd import hip as H
    y, mean, rstd = Buf(rows * D, y_dtype), Buf(rows), Buf(rows)
    H.check(H.lib.evk_layernorm_fwd(dptr(x_d), dcode(x_dtype), y.ptr, dcode(y_dtype), dptr(g), dptr(b), dptr(dg_d), dptr(db_d),
                                    dcode(d_dtype), mean.ptr, rstd.ptr, rows, D, mode, eps, H.stream()), 'layernorm_fwd')
    return y, mean, rstd


def test_layernorm_forward_edges():
    """evk_layernorm_fwd for 1 .. 2053 rows and D = 8 (one lane), 520 (nch = 65: one lane in the second chunk), 2040, 2048, both modes, with and
    without per-row deltas, x / y in f32 and 16 bits: y, mean and rstd against float64 on randn rows, on 1000 + randn (a one-pass variance would
    lose every digit) and with constant rows, which must give y = beta (+ delta) exactly -- no NaN from 0 * rstd in either mode."""
    w = Worst('layernorm_fwd')
    i = 0
    for sweep in range(2):
        for rows in LN_ROWS:
            for D in LN_D:
                i += 1
                j = i + 3 * sweep
                mode, deltas = j % 2, (j // 2) % 2 == 1
                x_dtype, y_dtype, d_dtype = (F32, BF)[(j // 4) % 2], (F32, BF)[(j // 8) % 2 ^ sweep], (BF, F32)[j % 3 == 0]
                kind = ('randn', 'offset', 'const')[j % 3]
                eps = 1e-5 if mode == 0 else 1e-6
                x = randn(rows, D, seed=i)
                if kind == 'offset':
                    x = x + 1000
                if kind == 'const':
                    x[0], x[-1] = 3.25, 3.25
                g, b, dg, db = _ln_params(rows, D, deltas, 50 + i)
                xd, xr = up(x, x_dtype)
                dgd, dgr = up(dg, d_dtype) if deltas else (None, None)
                dbd, dbr = up(db, d_dtype) if deltas else (None, None)
                y, mean, rstd = _ln_fwd(xd, x_dtype, y_dtype, g.cuda(), b.cuda(), dgd, dbd, d_dtype, rows, D, mode, eps)
                want, mu, r, _ = R.layernorm(xr, g, b, eps, mode, dgr, dbr)
                what = 'rows=%d D=%d mode=%d deltas=%d x %s y %s %s' % (rows, D, mode, deltas, x_dtype, y_dtype, kind)
                extra = 4 * R.spacing_f32(float(xr.abs().max())) if kind == 'offset' else 0.0
                got = y.cpu(rows, D)
                # an uncertainty of the inputs (and of their mean) reaches y = (x - mu) rstd (g + dg) + b multiplied by rstd |g + dg|
                gg = g.to(F64) + (dgr.to(F64) if deltas else 0)
                gain = r[:, None] * gg.abs()
                if y_dtype == F32:
                    w(what + ' y', got, want, R.f32_tol(want, extra * gain))
                else:
                    # f32 rounding of x - mu (relative to the row's largest |x|, times the gain) and of the product and the sum
                    xmax = xr.to(F64).abs().max(-1, keepdim=True).values
                    bb64 = b.to(F64) + (dbr.to(F64) if deltas else 0)
                    w(what + ' y', got, want, tol16(want, 4 * EPS * (gain * xmax + (want - bb64).abs() + bb64.abs())), ulps=True)
                w(what + ' mean', mean.cpu(), mu, R.f32_tol(mu, extra))
                w(what + ' rstd', rstd.cpu(), r, R.f32_tol(r))
                if kind == 'const':
                    bb = b if not deltas else b + dbr.float()
                    for row in (0, rows - 1):
                        wb = (bb if bb.dim() == 1 else bb[row]).to(y_dtype)
                        assert bool((got[row] == wb).all()), what + ': a constant row must give beta exactly'
    w.done('(f32: 1e-5 + 1e-5 |y| [+ 4 spacing(max |x|) rstd |g| at offset 1000]; 16-bit: 1 ulp + 2^-22 (rstd |g| max |x| + |xhat g| + |b|))')


def test_layernorm_backward_beyond_the_grid_cap():
    """evk_layernorm_bwd: its grid is capped at 512 blocks of 4 rows, so rows 2048 .. 2052 are reached by the grid-stride loop only -- the NaN
    pre-fill of dx shows a skipped row.  dx, ddgam and ddbet per row against float64 autograd; dbeta from integer-valued dy onto a non-zero
    start EXACTLY; dgamma within the accumulation bound 2 n 2^-24 sum |terms| of the float64 terms (n = rows + 1: the start value is a term) plus,
    per term dy * xhat, its own f32 rounding 2^-22 |dy| (|xhat| + rstd |x|) (xhat comes from the f32 mean and rstd; measured without it:
    4.2e-7 against 3.3e-7 at rows = 3).  16-bit dx and ddgam: one ulp plus the f32 rounding of their operands."""
    from evoke_amd import hip as H
    w = Worst('layernorm_bwd')
    i = 0
    for rows in LN_ROWS:
        for D in LN_D:
            i += 1
            mode, deltas = i % 2, (i // 2) % 2 == 1
            x_dtype, dy_dtype, dx_dtype, d_dtype = (F32, BF)[(i // 4) % 2], (BF, F32)[i % 3 == 0], (F32, BF)[(i // 3) % 2], (BF, F32)[(i // 5) % 2]
            eps = 1e-5 if mode == 0 else 1e-6
            x = randn(rows, D, seed=i) * (1.0 if i % 2 else 2.0) + (0.0 if i % 4 else 3.0)
            dy = torch.randint(-4, 5, (rows, D), generator=gen(200 + i)).float()
            g, b, dg, db = _ln_params(rows, D, deltas, 50 + i)
            xd, xr = up(x, x_dtype)
            dyd, dyr = up(dy, dy_dtype)
            dgd, dgr = up(dg, d_dtype) if deltas else (None, None)
            dbd, _ = up(db, d_dtype) if deltas else (None, None)
            gd = g.cuda()
            _, mean, rstd = _ln_fwd(xd, x_dtype, F32, gd, b.cuda(), dgd, dbd, d_dtype, rows, D, mode, eps)
            start_g, start_b = 0.5 + 0.01 * (torch.arange(D) % 7).float(), 3.0 + (torch.arange(D) % 4).float()
            with_sums = i % 5 != 0                        # dgamma / dbeta are optional (as a pair)
            dx = Buf(rows * D, dx_dtype)
            dgam_acc, dbet_acc = Buf.of(start_g), Buf.of(start_b)
            ddg, ddb = (Buf(rows * D, d_dtype), Buf(rows * D, d_dtype)) if deltas else (None, None)
            H.check(H.lib.evk_layernorm_bwd(dptr(dyd), dcode(dy_dtype), dptr(xd), dcode(x_dtype), dptr(gd), dptr(dgd), dcode(d_dtype), mean.ptr,
                                            rstd.ptr, dx.ptr, dcode(dx_dtype), dgam_acc.ptr if with_sums else None,
                                            dbet_acc.ptr if with_sums else None, ddg.ptr if deltas else None, ddb.ptr if deltas else None, rows, D,
                                            mode, eps, H.stream()), 'layernorm_bwd')
            xg = xr.to(F64).requires_grad_(True)
            yr, _, rr, xh = R.layernorm(xg, g, b, eps, mode, dgr, None)
            rr = rr.detach()
            yr.backward(dyr.to(F64))
            what = 'rows=%d D=%d mode=%d deltas=%d x %s dy %s dx %s' % (rows, D, mode, deltas, x_dtype, dy_dtype, dx_dtype)
            xh = xh.detach()
            terms = dyr.to(F64) * xh
            if dx_dtype == F32:
                w(what + ' dx', dx.cpu(rows, D), xg.grad, R.f32_tol(xg.grad))
            else:
                # dx = rstd (g - mean g) - xhat k2 with g = dy gamma, k2 ~ rstd mean(g xhat): 16 EPS of the magnitudes of the three terms
                gj = (dyr.to(F64) * (g.to(F64) + (dgr.to(F64) if deltas else 0))).abs()
                T = rr[:, None] * (gj + gj.mean(-1, keepdim=True) + xh.abs() * (gj * xh.abs()).mean(-1, keepdim=True) * D / (D - 1))
                w(what + ' dx', dx.cpu(rows, D), xg.grad, tol16(xg.grad, 16 * EPS * T), ulps=True)
            # one term dy xhat in f32: xhat = (x - mean) rstd carries the rounding of x - mean, relative to |x|, and of rstd
            term_tol = 4 * EPS * dyr.to(F64).abs() * (xh.abs() + rr[:, None] * xr.to(F64).abs())
            if with_sums:
                assert bool((dbet_acc.cpu().to(F64) == start_b.to(F64) + dyr.to(F64).sum(0)).all()), what + ': dbeta of integer-valued dy must be exact'
                bound = term_tol.sum(0) + 2 * (rows + 1) * EPS * (terms.abs().sum(0) + start_g.to(F64))
                w(what + ' dgamma', dgam_acc.cpu(), start_g.to(F64) + terms.sum(0), bound)
            else:
                assert bool((dbet_acc.cpu() == start_b).all()) and bool((dgam_acc.cpu() == start_g).all())
            if deltas:
                if d_dtype == F32:
                    w(what + ' ddgam', ddg.cpu(rows, D), terms, R.f32_tol(terms))
                else:
                    w(what + ' ddgam', ddg.cpu(rows, D), terms, tol16(terms, term_tol), ulps=True)
                assert bool((ddb.cpu(rows, D).to(F64) == dyr.to(F64)).all()), what + ': ddbet must be dy'
    w.done('(dx, ddgam f32: 1e-5 + 1e-5 |.|, 16-bit: 1 ulp + f32 rounding of the operands; dgamma: 2 n 2^-24 sum |terms| + per-term rounding; dbeta, ddbet: exact)')


# =============================================================================================================== D. log-softmax / NLL
LSM_V = [1, 63, 64, 65, 1445, 1536, 1537, 5000]
LSM_KINDS = ['randn4', 'offset', 'dominant', 'ninf', 'equal']


def _lsm_logits(kind, rows, V, seed):
    x = 4 * randn(rows, V, seed=seed)
    if kind == 'offset':
        x = x + 3e4
    elif kind == 'dominant':
        x[torch.arange(rows), torch.randint(0, V, (rows,), generator=gen(seed + 1))] += 80 + 20
    elif kind == 'ninf':
        x = x.masked_fill(torch.rand(rows, V, generator=gen(seed + 1)) < 0.3, -INF)
        x[:, (seed * 7) % V] = 0.5                     # every row keeps a finite entry
    elif kind == 'equal':
        x = torch.full((rows, V), 2.0)
    return x


def test_log_softmax_nll_family_edges():
    """evk_log_softmax_nll_fwd, evk_log_softmax_nll_rows and evk_nll_bwd at V around the 64-lane width and the 1536-column limit of the
    register kernel (V = 1537 and 5000 take the scanning kernel, here WITH targets), ld = pad8(V) with NaN pads, 1 / 5 / 300 rows, logits that
    are spread, offset by 3e4, dominated by one column, -inf in 30 % of the columns (what the HF logits processors produce) or all equal."""
    from evoke_amd import hip as H
    w = Worst('log_softmax / nll')
    i = 0
    for V in LSM_V:
        for kind in LSM_KINDS:
            for rep in range(2):
                i += 1
                rows = (1, 5, 300)[i % 3]
                ld = pad8(V)
                ld_out = V if rep else ld
                x = _lsm_logits(kind, rows, V, seed=i)
                full = torch.full((rows, ld), NAN)
                full[:, :V] = x
                fin = torch.isfinite(x)
                tgt = torch.multinomial(fin.float(), 1, generator=gen(300 + i))[:, 0]          # a finite column of each row
                wm = torch.tensor([0.0, 1.0, 2.5])[torch.randint(0, 3, (rows,), generator=gen(400 + i))]
                if rows > 1:
                    wm[0], wm[1] = 0.0, 1.0
                xd, td, wd = full.cuda(), tgt.cuda(), wm.cuda()
                logp, lse, acc = Buf(rows * ld_out), Buf(rows), Buf.of(torch.tensor([3.5, 1.25]))
                H.check(H.lib.evk_log_softmax_nll_fwd(dptr(xd), logp.ptr, lse.ptr, dptr(td), dptr(wd), acc.ptr, rows, V, ld, ld_out, H.stream()))
                want, wlse = R.log_softmax(x)
                what = 'V=%d %s rows=%d ld_out=%d' % (V, kind, rows, ld_out)
                extra = 4 * R.spacing_f32(float(x[fin].abs().max())) if kind == 'offset' else 0.0
                got = logp.cpu(rows, ld_out)
                assert bool((got[:, :V][~fin] == -INF).all()) and bool(torch.isfinite(got[:, :V][fin]).all()), what + ': -inf in, -inf out, finite elsewhere'
                w(what + ' logp', got[:, :V][fin], want[fin], R.f32_tol(want[fin], extra))
                assert bool(torch.isnan(got[:, V:]).all()), what + ': pad columns of logp must keep the sentinel'
                lse_c = lse.cpu()
                w(what + ' lse', lse_c, wlse, R.f32_tol(wlse, extra))
                nll = -want[torch.arange(rows), tgt] * wm.to(F64)
                # one term -(x_t - lse) w in f32: lse and the difference are rounded at the magnitude of the row's largest |x| (4 spacings with the log), and
                # the product adds a few EPS of |logp|
                big = torch.maximum(x.masked_fill(~fin, 0).abs().max(-1).values.to(F64), wlse.abs())
                terms_tol = (wm.to(F64) * (4 * R.ulp(big, F32) + 4 * EPS * (4 + want[torch.arange(rows), tgt].abs()))).sum()
                acc_c = acc.cpu()
                w(what + ' acc2[0]', acc_c[0], 3.5 + nll.sum(), terms_tol + 2 * (rows + 1) * 2.0 ** -24 * (nll.abs().sum() + 3.5))
                assert float(acc_c[1]) == 1.25 + float(wm.sum()), what + ': the sum of the weights is exact in f32'
                # all-zero weights leave the accumulator bit-identical
                acc0 = Buf.of(torch.tensor([3.5, 1.25]))
                H.check(H.lib.evk_log_softmax_nll_fwd(dptr(xd), None, None, dptr(td), dptr(torch.zeros(rows)), acc0.ptr, rows, V, ld,
                                                      ld, H.stream()))
                assert acc0.cpu().tolist() == [3.5, 1.25], what + ': zero weights must not touch acc2'
                # per-row entry point: the same lse bits, 0 where w == 0
                lse2, rown = Buf(rows), Buf(rows)
                H.check(H.lib.evk_log_softmax_nll_rows(dptr(xd), lse2.ptr, dptr(td), dptr(wd), rown.ptr, rows, V, ld, H.stream()))
                assert torch.equal(lse2.cpu().view(torch.int32), lse_c.view(torch.int32)), what + ': the two entry points disagree on lse'
                rn = rown.cpu()
                w(what + ' row nll', rn, nll, R.f32_tol(nll, extra * 2.5))
                assert bool((rn[wm == 0] == 0).all()) and not bool(torch.signbit(rn[wm == 0]).any()), what + ': rows with w = 0 must be exactly 0'
                # backward: (softmax - onehot) w gscale in 16 bits, pads and w = 0 rows exactly 0
                gs = 0.37
                ldo = ld if rep else ld + 8
                dl = Buf(rows * ldo, BF)
                H.check(H.lib.evk_nll_bwd(dptr(xd), lse.ptr, dptr(td), dptr(wd), dptr(torch.tensor([gs])), dl.ptr, rows, V, ld, ldo,
                                          H.stream()))
                sm = torch.exp(want)
                sm[torch.arange(rows), tgt] -= 1
                kk = wm.to(F64)[:, None] * float(torch.tensor(gs))
                wg = sm * kk
                gd = dl.cpu(rows, ldo)
                # exp(x - lse) in f32: lse and x - lse are rounded at the magnitude of the row's largest |x| (2 spacings), log and exp add a few
                # EPS relative to |logp|; exp turns all of it into a RELATIVE error of the probability.  Where nothing cancels this is far
                # below one ulp; at the target column it is what is left of softmax - 1
                rel = 2 * R.ulp(big, F32)[:, None] + 4 * EPS * (4 + torch.where(fin, want, torch.zeros_like(want)).abs())
                # ... and the fast exponential flushes what falls below the smallest normal f32 (include/evoke_hip.h says so)
                w(what + ' dlogits', gd[:, :V], wg, tol16(wg, torch.exp(want) * kk.abs() * rel + 2.0 ** -126 * kk.abs()), ulps=True)
                assert bool((gd[:, V:] == 0).all()) and bool((gd[wm == 0] == 0).all()), what + ': pads and w = 0 rows of dlogits must be 0'
    w.done('(f32: 1e-5 + 1e-5 |.| [+ 4 spacing(3e4) at the offset]; dlogits: 1 ulp + softmax w gscale (2 spacing(max |x|) + 2^-22 (4 + |logp|)))')


@pytest.mark.parametrize('V', [1536, 1537])
def test_log_softmax_scaled_either_side_of_the_register_limit(V):
    from evoke_amd import hip as H
    rows, ld, scale = 5, pad8(V) + 8, 0.5
    x = _lsm_logits('ninf', rows, V, seed=V)
    full = torch.full((rows, ld), NAN)
    full[:, :V] = x
    out = Buf(rows * ld)
    H.check(H.lib.evk_log_softmax_scaled(dptr(full), out.ptr, rows, V, ld, ld, scale, H.stream()))
    got, (want, _) = out.cpu(rows, ld), R.log_softmax(x, scale)
    fin = torch.isfinite(x)
    assert bool((got[:, :V][~fin] == -INF).all()) and bool(torch.isnan(got[:, V:]).all())
    w = Worst('log_softmax_scaled V=%d' % V)
    w('logp', got[:, :V][fin], want[fin], R.f32_tol(want[fin]))
    w.done()


# =============================================================================================================== E. top-k
TOPK_N = [0, 8, 255, 256, 257, 2049, 5784]           # 0 stands for n == k
TOPK_KINDS = ['five', 'equal', 'ninf', 'pinf', 'ascending', 'lane5']


def _topk_data(kind, rows, n, k, seed):
    if kind == 'five':
        return torch.tensor([-1.5, 0.0, 0.25, 2.0, 7.0])[torch.randint(0, 5, (rows, n), generator=gen(seed))]
    if kind == 'equal':
        return torch.full((rows, n), 1.25)
    if kind == 'ninf':                                # all -inf except k - 2 entries
        x = torch.full((rows, n), -INF)
        for r in range(rows):
            at = torch.randperm(n, generator=gen(seed + r))[:max(k - 2, 0)]
            x[r, at] = torch.randn(len(at), generator=gen(seed + r))
        return x
    x = randn(rows, n, seed=seed)
    if kind == 'pinf':
        x[:, (seed * 3) % n] = INF
        x[:, (seed * 5 + 1) % n] = INF
        x[:, (seed * 11 + 2) % n] = -INF
    elif kind == 'ascending':
        x = torch.arange(n, dtype=F32).repeat(rows, 1) * 0.5 - 7
    elif kind == 'lane5':                             # all winners in the local list of thread 5
        x[:, 5:5 + 256 * 8:256] = 100 + torch.arange(8, dtype=F32).flip(0) * (1 if seed % 2 else 0)
    return x


def test_topk_rows_ties_infinities_and_single_thread_winners():
    """evk_topk_rows against a stable descending float64 sort: values AND indices exactly -- `ties -> lowest index first` is what makes the
    beam search follow the reference."""
    from evoke_amd import hip as H
    i = cases = 0
    for n0 in TOPK_N:
        for k in (1, 2, 5, 8):
            for kind in TOPK_KINDS:
                n = n0 or k
                if kind == 'lane5' and n < 5 + 256 * 7 + 1:
                    continue
                i += 1
                rows = 300 if i % 6 == 2 else (1, 3)[i % 2]
                x = _topk_data(kind, rows, n, k, seed=i)
                vals, idx = Buf(rows * k, F32, 123.0), Buf(rows * k, torch.int64, 123)
                H.check(H.lib.evk_topk_rows(dptr(x), vals.ptr, idx.ptr, rows, n, k, H.stream()), 'topk_rows')
                wv, wi = R.topk_rows(x, k)
                gv, gi = vals.cpu(rows, k), idx.cpu(rows, k)
                what = 'n=%d k=%d rows=%d %s' % (n, k, rows, kind)
                assert torch.equal(gi, wi), '%s: indices differ, first row %r != %r' % (what, gi[0].tolist(), wi[0].tolist())
                assert bool((gv.to(F64) == wv).all()), what + ': values differ'
                cases += 1
    print('topk_rows: %d cases, values and indices exact' % cases)


def test_topk_rows_rejects_bad_arguments_without_writing():
    from evoke_amd import hip as H
    x = randn(3, 20, seed=1).cuda()
    vals, idx = Buf(3 * 8, F32, 123.0), Buf(3 * 8, torch.int64, 123)
    for args in ((dptr(x), vals.ptr, idx.ptr, 3, 20, 0), (dptr(x), vals.ptr, idx.ptr, 3, 20, 9), (dptr(x), vals.ptr, idx.ptr, 3, 4, 5),
                 (None, vals.ptr, idx.ptr, 3, 20, 2), (dptr(x), None, idx.ptr, 3, 20, 2), (dptr(x), vals.ptr, None, 3, 20, 2)):
        assert H.lib.evk_topk_rows(*args, H.stream()) == -1, args[3:]
    torch.cuda.synchronize()
    assert bool((vals.cpu() == 123).all()) and bool((idx.cpu() == 123).all())


# =============================================================================================================== F. activations
def _act_call(fn, *ptrs, n, act):
    from evoke_amd import hip as H
    H.check(fn(*ptrs, n, act, H.stream()))


@pytest.mark.parametrize('name', ['relu', 'gelu', 'tanh', 'sigmoid', 'gelu_new'])
def test_activation_forward_over_every_finite_pattern(name):
    """evk_act_fwd on every finite value of the storage format in one launch, against the float64 function: within one unit in the last place
    of the storage format (subnormal spacing at the bottom) -- the tails included, where 1 + erf(x / sqrt 2) and 1 + tanh(u) cancel."""
    from evoke_amd import hip as H
    x = R.finite_values(BF)
    y = Buf(x.numel(), BF)
    _act_call(H.lib.evk_act_fwd, dptr(x), y.ptr, n=x.numel(), act=R.ACTS[name])
    want = R.act(x, name)
    w = Worst('act_fwd %s' % name)
    w('y', y.cpu(), want, tol16(want))
    w.done('(1 ulp of %s; %d values)' % (BF, x.numel()))


@pytest.mark.parametrize('name', ['relu', 'gelu', 'tanh', 'sigmoid', 'gelu_new'])
def test_activation_backward_against_the_float64_derivative(name):
    """evk_act_bwd called directly, dx = dy act'(ref) for dy = 1 and -1.5: ref runs over every finite pattern (GELU, GELU_NEW: the
    pre-activation; RELU: the output), every pattern in [-1, 1] for TANH and in [0, 1] for SIGMOID (the output).  1 - r^2, r (1 - r) and the
    step are exact in f32: one ulp; the GELU derivatives cross zero near -0.75: one ulp plus 2^-21 of the magnitudes of their terms."""
    from evoke_amd import hip as H
    ref = R.finite_values(BF)
    if name == 'tanh':
        ref = ref[ref.float().abs() <= 1]
    if name == 'sigmoid':
        ref = ref[(ref.float() >= 0) & (ref.float() <= 1)]
    n = ref.numel()
    w = Worst('act_bwd %s' % name)
    for dyv in (1.0, -1.5):
        dx = Buf(n, BF)
        _act_call(H.lib.evk_act_bwd, dptr(torch.full((n,), dyv, dtype=BF)), dptr(ref), dx.ptr, n=n, act=R.ACTS[name])
        want = dyv * R.act_grad(ref, name)
        term = None
        r = ref.to(F64)
        if name == 'gelu':            # Phi(r) + r phi(r), Phi as 0.5 + 0.5 erf: 8 EPS of the magnitudes of the three terms
            term = abs(dyv) * 8 * EPS * (1 + (r * torch.exp(-0.5 * r * r)).abs() / math.sqrt(2 * math.pi))
        if name == 'gelu_new':        # 0.5 + 0.5 th + T2, T2 = 0.5 r (1 - th^2) K0 (1 + 3 K1 r^2): 1 - th^2 carries 8 EPS absolute (tanhf near +-1) while |u| < 12
            u = R.K0 * (r + R.K1 * r ** 3)
            fac = torch.where(u.abs() < 12, 0.5 * r.abs() * R.K0 * (1 + 3 * R.K1 * r * r), torch.zeros_like(r))
            T2 = R.act_grad(ref, name) - R._sigmoid(2 * u)
            term = abs(dyv) * (8 * EPS * (1 + T2.abs()) + 8 * EPS * fac)
        w('dy=%g' % dyv, dx.cpu(), want, tol16(want, term), ulps=term is not None)
    w.done('(%d values)' % n)


def test_activation_grid_stride_loop():
    """n = 8192 * 256 + 257: one element more than a full grid of 8192 blocks can take in one pass, plus a ragged tail"""
    from evoke_amd import hip as H
    v = R.finite_values(BF)
    n = 8192 * 256 + 257
    x = v.cuda().repeat(n // v.numel() + 1)[:n].contiguous()
    small = Buf(v.numel(), BF)
    _act_call(H.lib.evk_act_fwd, dptr(v), small.ptr, n=v.numel(), act=R.ACTS['gelu_new'])
    y, dx = Buf(n, BF), Buf(n, BF)
    _act_call(H.lib.evk_act_fwd, dptr(x), y.ptr, n=n, act=R.ACTS['gelu_new'])
    _act_call(H.lib.evk_act_bwd, dptr(x), dptr(x), dx.ptr, n=n, act=R.ACTS['relu'])
    want = small.t.repeat(n // v.numel() + 1)[:n]
    y.cpu(), dx.cpu()                                  # guard bands
    assert torch.equal(y.t.view(torch.int16), want.view(torch.int16)), 'the grid-stride pass differs from the single-pass result'
    assert bool((dx.t.float() == x.float().clamp_min(0)).all())


# =============================================================================================================== G. cast
def _cast(src, dst, n):
    from evoke_amd import hip as H
    H.check(H.lib.evk_cast(dptr(src), dcode(src.dtype), dst.ptr, dcode(dst.t.dtype), n, H.stream()), 'cast')


def _same_or_both_nan(got, want):
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    bits = torch.int16 if got.element_size() == 2 else torch.int32
    return bool((gn == wn).all()) and torch.equal(got.view(bits)[~wn], want.view(bits)[~wn])


def test_cast_is_round_to_nearest_even_and_bit_exact():
    """evk_cast writes every 16-bit weight shadow and the reducer's wire format.  16 -> 32: all 65536 patterns bit-equal to torch (NaN stays
    NaN).  32 -> 16: every finite storage value, every tie between neighbours and one f32 step either side of it, +-0, +-inf, NaN, f32
    subnormals and values past the largest finite one, bit-equal to torch's CPU conversion (any NaN for NaN).  32 -> 32 is a bit copy."""
    allp = R.all_patterns(BF)
    out = Buf(65536, F32)
    _cast(allp.cuda(), out, 65536)
    assert _same_or_both_nan(out.cpu(), allp.float()), '16 -> 32 differs from torch'
    probes = torch.cat([R.rne_probes(BF), R.cast_specials()])
    want = probes.to(BF)
    out = Buf(probes.numel(), BF)
    _cast(probes.cuda(), out, probes.numel())
    got = out.cpu()
    bad = ~((got.view(torch.int16) == want.view(torch.int16)) | (torch.isnan(got.float()) & torch.isnan(want.float())))
    assert not bool(bad.any()), '32 -> 16: %d of %d probes differ from round-to-nearest-even, first: %r -> %r, want %r' % (
        int(bad.sum()), bad.numel(), float(probes[bad][0]), float(got[bad][0]), float(want[bad][0]))
    out = Buf(probes.numel(), F32)
    _cast(probes.cuda(), out, probes.numel())
    assert torch.equal(out.cpu().view(torch.int32), probes.view(torch.int32)), '32 -> 32 is not a bit copy'
    print('cast: 65536 patterns up, %d probes down, bit-exact' % probes.numel())


def test_cast_tails_and_grid_stride_loop():
    """n = 1 .. 7 (the n & 3 tail, written by block 0 alone) and n = 8192 * 256 * 4 + 3 (one vector more than the grid takes in one pass)"""
    probes = R.rne_probes(BF)
    tab16 = probes.to(BF)
    for n in (1, 2, 3, 4, 5, 7):
        for src, want, ddt in ((probes[40000:40000 + n], tab16[40000:40000 + n], BF), (tab16[300:300 + n], tab16[300:300 + n].float(), F32),
                               (probes[5:5 + n], probes[5:5 + n], F32)):
            out = Buf(8, ddt)
            _cast(src.contiguous().cuda(), out, n)
            got = out.cpu()
            assert _same_or_both_nan(got[:n], want) and bool(torch.isnan(got[n:].float()).all()), 'n = %d -> %s' % (n, ddt)
    n = 8192 * 256 * 4 + 3
    reps = n // probes.numel() + 1
    src = probes.cuda().repeat(reps)[:n].contiguous()
    out = Buf(n, BF)
    _cast(src, out, n)
    out.cpu()
    assert torch.equal(out.t.view(torch.int16), tab16.cuda().repeat(reps)[:n].view(torch.int16)), 'the grid-stride pass of the cast differs'


# =============================================================================================================== H. column sums
def test_colsum_exact_on_integer_data_for_both_kernels_and_offset_pointers():
    """evk_colsum supplies every bias gradient.  Integer-valued 16-bit inputs in -4 .. 4 keep every partial sum below 2^24, so the f32 sums are
    exact in any order: equality.  ld = pad8(N) from the allocation takes the 16-byte kernel, ld = pad2(N), ld = 3 N and a base pointer offset
    by 2 elements (how layers.py reads one of three interleaved blocks) take the pair kernel.  Accumulated onto a non-zero out; NaN in the pad
    columns; an odd ld is refused."""
    from evoke_amd import hip as H
    cases = 0
    for M in (1, 7, 31, 32, 33, 1000, 4640):
        for N in (2, 8, 255, 256, 257, 1445):
            for ld in (pad8(N), N + (N & 1), 3 * N):
                for off in (0, 2):
                    start = (5 + torch.arange(N) % 3).float()
                    out = Buf.of(start)
                    if ld % 2:
                        x = torch.zeros(off + M * ld, dtype=BF, device='cuda')
                        assert H.lib.evk_colsum(x.data_ptr() + 2 * off, out.ptr, M, N, ld, H.stream()) == -1, 'an odd ld must be refused'
                        assert bool((out.cpu() == start).all())
                        continue
                    x = torch.full((off + M * ld,), NAN, dtype=BF, device='cuda')
                    body = x[off:].view(M, ld)
                    body[:, :N] = torch.randint(-4, 5, (M, N), device='cuda', generator=torch.Generator('cuda').manual_seed(M * 7 + N)).to(BF)
                    H.check(H.lib.evk_colsum(x.data_ptr() + 2 * off, out.ptr, M, N, ld, H.stream()), 'colsum')
                    want = start.to(F64) + body[:, :N].to(F64).sum(0).cpu()
                    got = out.cpu().to(F64)
                    assert bool((got == want).all()), 'M=%d N=%d ld=%d offset=%d: %d sums differ, worst by %g' % (
                        M, N, ld, off, int((got != want).sum()), float((got - want).abs().nan_to_num(nan=INF).max()))
                    cases += 1
    print('colsum: %d cases exact' % cases)


# =============================================================================================================== I. L2 norm, soft cross-entropy
@pytest.mark.parametrize('rows', [1, 4, 5, 257])
def test_l2norm_and_soft_cross_entropy_edges(rows):
    """evk_l2norm_fwd / _bwd and evk_softce for D / Cn = 1, 63, 64, 65, 2048: a zero row must come out as F.normalize(eps = 1e-12) gives it
    (forward), dx and dz against float64, the diagonal mask on and off, the loss accumulated onto a non-zero start."""
    from evoke_amd import hip as H
    w = Worst('l2norm / softce rows=%d' % rows)
    for D in (1, 63, 64, 65, 2048):
        x = randn(rows, D, seed=D + rows) * 3
        xz = x.clone()
        xz[0] = 0
        y, nrm = Buf(rows * D), Buf(rows)
        H.check(H.lib.evk_l2norm_fwd(dptr(xz), y.ptr, nrm.ptr, rows, D, H.stream()))
        wy, wn = R.l2norm(xz)
        w('D=%d y (zero row)' % D, y.cpu(rows, D), wy, R.f32_tol(wy))
        assert bool((y.cpu(rows, D)[0] == 0).all()) and float(nrm.cpu()[0]) == float(torch.tensor(1e-12, dtype=F32))
        y, nrm, dx = Buf(rows * D), Buf(rows), Buf(rows * D)
        dy = randn(rows, D, seed=D + rows + 1)
        H.check(H.lib.evk_l2norm_fwd(dptr(x), y.ptr, nrm.ptr, rows, D, H.stream()))
        H.check(H.lib.evk_l2norm_bwd(dptr(dy), y.ptr, nrm.ptr, dx.ptr, rows, D, H.stream()))
        xg = x.to(F64).requires_grad_(True)
        yr, nr = R.l2norm(xg)
        yr.backward(dy.to(F64))
        w('D=%d y' % D, y.cpu(rows, D), yr.detach(), R.f32_tol(yr.detach()))
        w('D=%d norm' % D, nrm.cpu(), nr.detach(), R.f32_tol(nr.detach()))
        w('D=%d dx' % D, dx.cpu(rows, D), xg.grad, R.f32_tol(xg.grad))
        for diag in (0, 1):
            Cn, scale, gs, start = D, 1.0 / rows, 0.7, 2.5
            z, t = 3 * randn(rows, Cn, seed=Cn + 7), torch.softmax(randn(rows, Cn, seed=Cn + 8), -1)
            if diag:
                idx = torch.arange(min(rows, Cn))
                t[idx, idx] = 0
            loss, dz = Buf.of(torch.tensor([start])), Buf(rows * Cn)
            H.check(H.lib.evk_softce(dptr(z), dptr(t), loss.ptr, dz.ptr, dptr(torch.tensor([gs])), rows, Cn, scale, diag,
                                     H.stream()))
            _, zm = R.softce(z, t, scale, diag)
            lp, _ = R.log_softmax(zm)
            per_row = -(t.to(F64) * lp).sum(-1) * scale
            # one row's (lse sum t - sum t z) scale in f32: lse is rounded at the magnitude of the row's largest |z| (4 spacings with the log), the two sums
            # carry a few EPS of sum |t z|; then the accumulation bound
            live = zm > -1e8
            zbig = torch.maximum((zm.abs() * live).max(-1).values, torch.where(live.any(-1), torch.logsumexp(zm, -1).abs(), torch.zeros(rows, dtype=F64)))
            row_tol = scale * (t.to(F64).sum(-1) * 4 * R.ulp(zbig, F32) + 16 * EPS * (t.to(F64) * zm * live).abs().sum(-1))
            tol = row_tol.sum() + 2 * (rows + 1) * EPS * (per_row.abs().sum() + start)
            w('Cn=%d diag=%d loss' % (Cn, diag), loss.cpu()[0], start + per_row.sum(), tol)
            wdz = (torch.exp(lp) * t.to(F64).sum(-1, keepdim=True) - t.to(F64)) * float(torch.tensor(gs)) * float(torch.tensor(scale))
            if diag:
                wdz[idx, idx] = 0
            gz = dz.cpu(rows, Cn)
            w('Cn=%d diag=%d dz' % (Cn, diag), gz, wdz, R.f32_tol(wdz))
            if diag:
                assert bool((gz[idx, idx] == 0).all())
    w.done('(f32: 1e-5 + 1e-5 |.|; loss: per-row rounding + 2 n 2^-24 sum |terms|)')
