"""Hop-by-hop fp64 audit of the native trunk runner (csrc/trunk.hip: evk_trunk_forward / evk_trunk_backward).

The runner keeps, per conv + batch-norm pair, the raw convolution output y, the activation z, the gradient dy, the statistics block
(sum, sumsq, scale, shift, mean, invstd) and the backward sums (sum_g, sum_gx) in its workspace until the backward has finished
(evk_trunk_plan gives the offsets).  So every layer is checked LOCALLY: take the engine's own stored inputs of one hop, redo that hop in
float64 with plain torch, compare with what the engine stored as the hop's output.  One hop carries one or two 16-bit roundings and one f32
accumulation whatever came before it, so the bounds below are a few units of 16-bit round-off and hold at any depth.

The restatement is written from the semantics of torchvision's Bottleneck as oracle/functional.py states them (conv -> batch norm -> ReLU,
identity / downsample added before the last ReLU, nn.BatchNorm2d's train / eval arithmetic and running-statistics update, 3x3 / stride-2 /
pad-1 max-pool behind the 7x7 / stride-2 / pad-3 stem), not from the kernels.

Bounds (derived, never fitted to what the engine gives).  u = 2^-11 (fp16 storage) or 2^-8 (bf16); f = 2^-24.
  * a 16-bit output of an f32 accumulation of K products:   |got - want| <= u |want| + K f (|a| (*) |b|) (+ half a subnormal step in fp16),
    (|a| (*) |b|) the same product evaluated on absolute values;
  * f32 outputs (weight gradients) get the accumulation term only, K = the number of rows summed;
  * z from the stored y is one rounding of three f32 operations;
  * an intermediate the engine rounds to 16 bits and the audit has unrounded (the dz between a data gradient and the batch-norm backward
    that reads it) is propagated through the hop's linear map (|scale| u |dz| on dy);
  * long column sums (sum, sumsq, sum_g, sum_gx, dgamma, dbeta): the root-sum-square model K_RSS * sqrt(sum r_t^2) over the per-term rounding
    magnitudes r_t (u |t| for a term read from a 16-bit tensor), K_RSS = 4, plus the per-term accumulation errors and M f sum|t| for the f32
    summation of M rows.  The same bound is used whether a route sums f32 accumulators or the stored 16-bit tensor;
  * mean / invstd / scale / shift: the bounds of sum and sumsq pushed through E[x^2] - mean^2, 1 / sqrt(var + eps) (interval form, so it
    stays valid where var + eps is tiny) and the affine map; rsqrtf and the few f32 operations get 4 f relative;
  * sum_gx of conv1 / conv2 of a bottleneck carries one more rounding per term where the gate-statistics route forms it from the stored z
    (gate_identity_term, with the code reference);
  * the block-input gradient is NOT kept by the runner (it rotates through six buffers), so the audit carries it in fp64 along the
    identity chain; its budget is stated next to the loop in audit_backward ("skip chain").
No bound here contains a constant measured on the engine.  tests/test_trunk_audit_cpu.py checks on the CPU that a plain fp32 evaluation of the
same hops (emulate_engine) satisfies every bound with no element left out, and that defects of a few per cent are named at their quantity.
"""
import ctypes as C
from collections import namedtuple

import torch
import torch.nn.functional as F

F32_EPS = 2.0 ** -24
K_RSS = 4.0
GUARD = 1 << 20
GUARD_BYTE = 0xA5

Check = namedtuple('Check', 'pair name got want bound')


def unit(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def tiny(dtype):
    """half the spacing of the subnormals: the absolute rounding error floor of the format (nothing to speak of in bf16)"""
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


# ---- fp64 hops (NHWC activations, [Co][KH][KW][Ci] weights: the engine's layouts) ---------------------------------------------------------
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def conv_mm(x, w, stride, pad):
    """the convolution from matmuls, slices and sums only: a pointwise convolution is one matmul, a KH x KW one is KH * KW shifted matmuls.
    The reference ON THE DEVICE (float64): neither the library under test nor a vendor convolution is trusted there; its data / weight
    gradients come from autograd over these same operations."""
    N, H, W, Ci = x.shape
    Co, KH, KW, _ = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
    out = None
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :]
            t = xs.reshape(-1, Ci) @ w[:, kh, kw, :].t()
            out = t if out is None else out + t
    return out.view(N, Ho, Wo, Co)


def conv64(x, w, stride, pad):
    if x.is_cuda:
        return conv_mm(x, w, stride, pad)
    return F.conv2d(_nchw(x), _nchw(w), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def dgrad64(dy, w, x_shape, stride, pad):
    n, h, ww, c = x_shape
    if dy.is_cuda:
        x = torch.zeros(x_shape, dtype=dy.dtype, device=dy.device, requires_grad=True)
        return torch.autograd.grad(conv_mm(x, w, stride, pad), x, dy)[0]
    return torch.nn.grad.conv2d_input((n, c, h, ww), _nchw(w), _nchw(dy), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def wgrad64(dy, x, w_shape, stride, pad):
    co, kh, kw, ci = w_shape
    if dy.is_cuda:
        w = torch.zeros(w_shape, dtype=dy.dtype, device=dy.device, requires_grad=True)
        return torch.autograd.grad(conv_mm(x, w, stride, pad), w, dy)[0]
    return torch.nn.grad.conv2d_weight(_nchw(x), (co, ci, kh, kw), _nchw(dy), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()


def maxpool3x3s2(x):
    """3x3 / stride 2 / pad 1 max-pool of [N][H][W][C] (H, W even) as the maximum of nine strided slices"""
    N, H, W, C_ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float('-inf'))
    out = None
    for kh in range(3):
        for kw in range(3):
            t = xp[:, kh:kh + H - 1:2, kw:kw + W - 1:2, :]
            out = t if out is None else torch.maximum(out, t)
    return out


def _to(dev, x):
    if isinstance(x, torch.Tensor):
        return x.to(dev)
    if isinstance(x, dict):
        return {k: _to(dev, v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_to(dev, v) for v in x)
    return x


def col_sum_bound(t, r, e, rows):
    """bound of an f32 column sum over `rows` rows of terms t whose 16-bit roundings have magnitude r (root-sum-square, K_RSS) and whose
    f32 accumulation errors are bounded by e (worst case), plus the f32 summation itself"""
    C_ = t.shape[-1]
    t, r, e = t.reshape(-1, C_), r.reshape(-1, C_), e.reshape(-1, C_)
    return K_RSS * (r * r).sum(0).sqrt() + e.sum(0) + rows * F32_EPS * t.abs().sum(0)


class Workspace:
    """typed views into the runner's workspace: a CPU copy of its bytes, or the device buffer itself (the audit runs where the bytes are)"""

    def __init__(self, raw, pairs, plan, store):
        self.raw, self.pairs, self.plan, self.store = raw, pairs, plan, store
        self.first = [i for i, p in enumerate(pairs) if p.role == 1]       # first pair index of every block
        self.down = [i + 3 < len(pairs) and pairs[i + 3].role == 4 for i in self.first]

    def view(self, off, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        nb = n * torch.empty(0, dtype=dtype).element_size()
        assert off >= 0 and off + nb <= self.raw.numel()
        return self.raw[off:off + nb].view(dtype).view(*shape)

    def act_shape(self, i):
        p = self.pairs[i]
        if i == 0:
            return (self.N, self.H // 2, self.W // 2, 64)
        return (p.g.N, p.g.Ho, p.g.Wo, p.C)

    def act(self, i, which):
        return self.view(getattr(self.pairs[i], which), self.act_shape(i), self.store)

    def stats(self, i):
        return self.view(self.pairs[i].stats, (6, self.pairs[i].C), torch.float32).double()

    def sums(self, i):
        return self.view(self.pairs[i].sums, (2, self.pairs[i].C), torch.float32).double()


def stored_tensors(ws, backward=True, training=True):
    """{name: bytes view} of everything the audit reads: what has to be bit-identical between a zero-filled and a NaN-filled workspace
    (eval mode leaves the sum / sumsq rows of the statistics block unwritten, and reads neither)"""
    out = {}
    P = ws.plan
    for n in ('xpad', 'wp', 'pooled', 'pool_idx'):
        out[n] = ws.raw[getattr(P, n):getattr(P, n) + getattr(P, n + '_bytes')]
    for i, p in enumerate(ws.pairs):
        names = [('y', p.act_bytes), ('z', p.act_bytes), ('stats', p.stats_bytes)]
        if backward:
            names += [('dy', p.act_bytes), ('sums', p.sums_bytes)]
        for n, nb in names:
            skip = 2 * 4 * p.C if n == 'stats' and not training else 0
            out['pair%d.%s' % (i, n)] = ws.raw[getattr(p, n) + skip:getattr(p, n) + nb]
    return out


# ---- the audit ----------------------------------------------------------------------------------------------------------------------------
def _block_input(ws, b):
    P = ws.plan
    if b == 0:
        return ws.view(P.pooled, (ws.N, ws.H // 4, ws.W // 4, 64), ws.store)
    return ws.act(ws.first[b - 1] + 2, 'z')


def _pair_input(ws, i):
    p = ws.pairs[i]
    b = p.block
    if p.role in (1, 4):
        return _block_input(ws, b)
    return ws.act(i - 1, 'z')


def audit_forward(ws, params, images, training, eps, momentum, running_before, running_after, out):
    """params[i]: dict(w, gamma, beta) CPU tensors (w: the 16-bit [Co][KH][KW][Ci] weight; pair 0: the f32 OIHW master of the stem);
    running_*[i]: (mean, var) before / after the forward.  Yields Check tuples."""
    u, tn, store = unit(ws.store), tiny(ws.store), ws.store
    P, N, H, W = ws.plan, ws.N, ws.H, ws.W
    dev = ws.raw.device
    params, images, running_before, running_after, out = (_to(dev, t) for t in (params, images, running_before, running_after, out))

    # stem operands: the packed image and the packed, rounded master weight -- exact
    xpad = ws.view(P.xpad, (N, H + 6, W + 8, 4), store)
    want = torch.zeros(N, H + 6, W + 8, 4, dtype=store, device=dev)
    want[:, 3:H + 3, 3:W + 3, :3] = images.permute(0, 2, 3, 1).to(store)
    yield Check(0, 'xpad', xpad.double(), want.double(), torch.zeros(()).double())
    wp = ws.view(P.wp, (64, 7, 8, 4), store)
    want = torch.zeros(64, 7, 8, 4, dtype=store, device=dev)
    want[:, :, :7, :3] = params[0]['w'].permute(0, 2, 3, 1).to(store)
    yield Check(0, 'wp', wp.double(), want.double(), torch.zeros(()).double())

    for i, p in enumerate(ws.pairs):
        gamma, beta = params[i]['gamma'].double(), params[i]['beta'].double()
        if i == 0:
            # [N][H+6][W+8][4] * [64][7][8][4], stride 2, no further padding: column W/2 of the result only sees padding and is dropped
            xin, wt = xpad.double(), wp.double()
            conv = conv64(xin, wt, 2, 0)[:, :, :W // 2].contiguous()
            aconv = conv64(xin.abs(), wt.abs(), 2, 0)[:, :, :W // 2].contiguous()
            K, relu, idt = 7 * 7 * 3, True, None
        else:
            g = p.g
            xin, wt = _pair_input(ws, i).double(), params[i]['w'].double()
            conv = conv64(xin, wt, g.stride_h, g.pad_h)
            aconv = conv64(xin.abs(), wt.abs(), g.stride_h, g.pad_h)
            K, relu, idt = g.KH * g.KW * g.Ci, p.role != 4, None
            if p.role == 3:
                b = p.block
                idt = (ws.act(i + 1, 'z') if ws.down[b] else _block_input(ws, b)).double()
        M = p.M
        eacc = K * F32_EPS * aconv
        y = ws.act(i, 'y').double()
        yield Check(i, 'y', y, conv, u * conv.abs() + eacc + tn)

        st = ws.stats(i)
        rm0, rv0 = (t.double() for t in running_before[i])
        rm1, rv1 = (t.double() for t in running_after[i])
        rel = 4 * F32_EPS
        if training:
            # statistics of the UNROUNDED convolution (the runner reduces f32 accumulators); a route that reduces the stored y is inside the
            # root-sum-square term
            s64, q64 = conv.reshape(M, -1).sum(0), (conv * conv).reshape(M, -1).sum(0)
            b_s = col_sum_bound(conv, u * conv.abs(), eacc, M)
            b_q = col_sum_bound(conv * conv, 2 * u * conv * conv, 2 * conv.abs() * eacc + eacc * eacc, M)
            yield Check(i, 'sum', st[0], s64, b_s)
            yield Check(i, 'sumsq', st[1], q64, b_q)
            mean = s64 / M
            b_mean = b_s / M + rel * mean.abs()
            ex2 = q64 / M
            var = (ex2 - mean * mean).clamp_min(0)
            b_var = b_q / M + 2 * mean.abs() * b_mean + b_mean * b_mean + rel * (ex2 + mean * mean)
            # nn.BatchNorm2d: running = (1 - momentum) * running + momentum * batch, the variance with Bessel's correction
            bess = M / max(M - 1.0, 1.0)
            want_rm, want_rv = (1 - momentum) * rm0 + momentum * mean, (1 - momentum) * rv0 + momentum * var * bess
            yield Check(i, 'running_mean', rm1, want_rm, momentum * b_mean + rel * (rm0.abs() + mean.abs()))
            yield Check(i, 'running_var', rv1, want_rv, momentum * bess * b_var + rel * (rv0.abs() + var * bess))
        else:
            mean, var = rm0, rv0
            b_mean = torch.zeros_like(mean)
            b_var = torch.zeros_like(var)
            yield Check(i, 'running_mean', rm1, rm0, torch.zeros(()).double())
            yield Check(i, 'running_var', rv1, rv0, torch.zeros(()).double())
        istd = (var + eps).rsqrt()
        lo, hi = (var + b_var + eps).rsqrt(), ((var - b_var).clamp_min(0) + eps).rsqrt()
        b_is = torch.maximum(hi - istd, istd - lo) + rel * hi
        scale, shift = gamma * istd, beta - mean * gamma * istd
        b_scale = gamma.abs() * b_is + rel * scale.abs()
        b_shift = gamma.abs() * (mean.abs() * b_is + (istd + b_is) * b_mean) + rel * (beta.abs() + (mean * scale).abs())
        yield Check(i, 'mean', st[4], mean, b_mean)
        yield Check(i, 'invstd', st[5], istd, b_is)
        yield Check(i, 'scale', st[2], scale, b_scale)
        yield Check(i, 'shift', st[3], shift, b_shift)

        # z from the engine's own stored y, scale, shift (+ stored identity): three f32 operations, one rounding
        pre = y * st[2] + st[3]
        mag = (y * st[2]).abs() + st[3].abs()
        if idt is not None:
            pre, mag = pre + idt, mag + idt.abs()
        zw = pre.clamp_min(0) if relu else pre
        yield Check(i, 'z', ws.act(i, 'z').double(), zw, u * pre.abs() + 3 * F32_EPS * mag + tn)

    # max-pool 3x3 / stride 2 / pad 1 of the stored stem activation: exact, and the recorded tap holds the maximum
    z0 = ws.act(0, 'z').double()
    pooled = ws.view(P.pooled, (N, H // 4, W // 4, 64), store).double()
    want = maxpool3x3s2(z0)
    yield Check(0, 'pooled', pooled, want, torch.zeros(()).double())
    ih, iw, ok = _pool_taps(ws)
    yield Check(0, 'pool_idx in range', ok.double(), torch.ones_like(ok).double(), torch.zeros(()).double())
    n_i = torch.arange(N, device=dev).view(N, 1, 1, 1).expand_as(ih)
    c_i = torch.arange(64, device=dev).view(1, 1, 1, 64).expand_as(ih)
    at = z0[n_i, ih.clamp(0, H // 2 - 1), iw.clamp(0, W // 2 - 1), c_i]
    yield Check(0, 'pool_idx holds the maximum', at, pooled, torch.zeros(()).double())
    last = ws.first[-1] + 2
    yield Check(last, 'out', out.double(), ws.act(last, 'z').double(), torch.zeros(()).double())


def _pool_taps(ws):
    """input coordinates the recorded max-pool taps point at (tap = kh * 3 + kw, ih = 2 oh - 1 + kh), and whether they are legal"""
    N, H2, W2 = ws.N, ws.H // 2, ws.W // 2
    idx = ws.view(ws.plan.pool_idx, (N, H2 // 2, W2 // 2, 64), torch.uint8).long()
    oh = torch.arange(H2 // 2, device=idx.device).view(1, -1, 1, 1)
    ow = torch.arange(W2 // 2, device=idx.device).view(1, 1, -1, 1)
    ih, iw = 2 * oh - 1 + idx // 3, 2 * ow - 1 + idx % 3
    ok = (idx < 9) & (ih >= 0) & (ih < H2) & (iw >= 0) & (iw < W2)
    return ih, iw, ok


def gate_identity_term(dz, z, gamma, u):
    """Rounding budget (squared, per channel) of sum_gx where it is formed from the gate statistics (sum g, sum g z) of a data-gradient
    epilogue through xhat = (z - beta) / gamma on the 16-bit STORED z (csrc/bn.hip, comment above EVK_GATE_RATIO: "a relative error of
    ~2^-11 |beta / gamma| in sum g*xhat"; conv1 / conv2 of every bottleneck): one more rounding per term, u |z| |g| / |gamma|.  Equal values
    of z round equally, so the terms of one value add up before the root-sum-square over the distinct values (a channel whose activation is
    constant has ONE rounding error, times sum g).  Channels with gamma = 0 take no such route (their sum is the exact one or zero)."""
    M, C_ = z.numel() // z.shape[-1], z.shape[-1]
    z2, g2 = z.reshape(M, C_), dz.reshape(M, C_)
    order = z2.argsort(0)
    zs, gs = z2.gather(0, order), g2.gather(0, order)
    new = torch.ones(M, C_, dtype=torch.bool, device=z.device)
    new[1:] = zs[1:] != zs[:-1]
    gid = new.long().cumsum(0) - 1 + torch.arange(C_, device=z.device).view(1, C_) * M            # one id per (channel, distinct value)
    grp = torch.zeros(M * C_, dtype=torch.float64, device=z.device).index_add_(0, gid.reshape(-1), (gs * zs.abs()).reshape(-1)).view(C_, M)
    safe = torch.where(gamma != 0, gamma.abs(), torch.ones_like(gamma))
    return torch.where(gamma != 0, (u * grp / safe.view(C_, 1)).pow(2).sum(1), torch.zeros_like(gamma))


def _bn_backward(ws, i, params, training, dz, R, A, grads_before, grads_after):
    """One batch-norm backward hop of pair i from the fp64 dz.  The engine read a 16-bit dz that differs from `dz` by at most R (roundings,
    root-sum-square in the column sums) + A (f32 accumulation, worst case) elementwise.  nn.BatchNorm2d backward: train mode through the batch
    statistics, dy = scale (dz - mean(dz) - xhat mean(dz xhat)); eval mode the fixed affine map dy = scale dz; dbeta = sum dz, dgamma =
    sum dz xhat in both.  xhat from the engine's stored y, mean, invstd."""
    u, tn = unit(ws.store), tiny(ws.store)
    p = ws.pairs[i]
    M, C_ = p.M, p.C
    st = ws.stats(i)
    scale, mean, istd = st[2], st[4], st[5]
    y = ws.act(i, 'y').double()
    xhat = (y - mean) * istd
    e_xhat = 3 * F32_EPS * (y.abs() + mean.abs()) * istd                 # the engine forms xhat in f32
    sg, sgx = dz.reshape(M, C_).sum(0), (dz * xhat).reshape(M, C_).sum(0)
    b_sg = col_sum_bound(dz, R, A, M)
    b_sgx = col_sum_bound(dz * xhat, R * xhat.abs(), A * xhat.abs() + (dz.abs() + R + A) * e_xhat, M)
    if p.role in (1, 2):
        b_sgx = b_sgx + K_RSS * gate_identity_term(dz, ws.act(i, 'z').double(), params[i]['gamma'].double(), u).sqrt()
    sums = ws.sums(i)
    yield Check(i, 'sum_g', sums[0], sg, b_sg)
    yield Check(i, 'sum_gx', sums[1], sgx, b_sgx)
    for name, want, bound in (('dbeta', sg, b_sg), ('dgamma', sgx, b_sgx)):
        if grads_before[i][name] is not None:
            g0, g1 = grads_before[i][name].double(), grads_after[i][name].double()
            yield Check(i, name + ' increment', g1 - g0, want, bound + 2 * F32_EPS * (g0.abs() + g1.abs()))
    if training:
        want = scale * (dz - sg / M - xhat * (sgx / M))
        Bc = scale * istd * sgx / M
        Cc = scale * (mean * istd * sgx / M - sg / M)
        mag = (scale * dz).abs() + (Bc * y).abs() + Cc.abs()           # dy = A g + B x + C per channel in f32 (bn.hip: bn_bwd_apply_kernel)
        prop = scale.abs() * (R + A + b_sg / M + xhat.abs() * b_sgx / M)
    else:
        want = scale * dz
        mag = want.abs()
        prop = scale.abs() * (R + A)
    yield Check(i, 'dy', ws.act(i, 'dy').double(), want, u * want.abs() + prop + 4 * F32_EPS * mag + tn)


def _dgrad(ws, i, params, gate):
    """gate * (data gradient of pair i from its stored dy), the f32 accumulation bound of the same product"""
    g = ws.pairs[i].g
    dy, wt = ws.act(i, 'dy').double(), params[i]['w'].double()
    shape = (g.N, g.Hi, g.Wi, g.Ci)
    d = dgrad64(dy, wt, shape, g.stride_h, g.pad_h)
    a = g.Co * g.KH * g.KW * F32_EPS * dgrad64(dy.abs(), wt.abs(), shape, g.stride_h, g.pad_h)
    if gate is not None:
        m = (gate > 0).double()
        d, a = d * m, a * m
    return d, a


def _wgrad_check(ws, i, params, xin, grads_before, grads_after):
    p = ws.pairs[i]
    if grads_before[i]['dw'] is None:
        return
    dy = ws.act(i, 'dy').double()
    g0, g1 = grads_before[i]['dw'].double(), grads_after[i]['dw'].double()
    if i == 0:
        N, H, W = ws.N, ws.H, ws.W
        dyp = F.pad(dy, (0, 0, 0, 1))                 # the dropped output column W/2 (see audit_forward) carries no gradient
        want = wgrad64(dyp, xin, (64, 7, 8, 4), 2, 0)[:, :, :7, :3].permute(0, 3, 1, 2)          # -> OIHW, the master's layout
        absw = wgrad64(dyp.abs(), xin.abs(), (64, 7, 8, 4), 2, 0)[:, :, :7, :3].permute(0, 3, 1, 2)
    else:
        g = p.g
        shape = (g.Co, g.KH, g.KW, g.Ci)
        want = wgrad64(dy, xin, shape, g.stride_h, g.pad_h)
        absw = wgrad64(dy.abs(), xin.abs(), shape, g.stride_h, g.pad_h)
    yield Check(i, 'dW increment', g1 - g0, want, p.M * F32_EPS * absw + 2 * F32_EPS * (g0.abs() + g1.abs()))


def audit_backward(ws, params, dout, training, grads_before, grads_after):
    """grads_*[i]: dict(dw, dgamma, dbeta) of CPU f32 tensors before / after the backward (None = frozen).  Yields Check tuples."""
    u, tn = unit(ws.store), tiny(ws.store)
    nb = len(ws.first)
    last = ws.first[-1] + 2
    dev = ws.raw.device
    params, dout, grads_before, grads_after = (_to(dev, t) for t in (params, dout, grads_before, grads_after))
    # gradient w.r.t. the last block's output behind its ReLU: a masked copy of dout, exact
    G = dout.double() * (ws.act(last, 'z').double() > 0)
    R, A = torch.zeros_like(G), torch.zeros_like(G)
    for b in range(nb - 1, -1, -1):
        i = ws.first[b]
        X = _block_input(ws, b).double()
        yield from _bn_backward(ws, i + 2, params, training, G, R, A, grads_before, grads_after)
        z1, z0 = ws.act(i + 1, 'z').double(), ws.act(i, 'z').double()
        S1, A1 = _dgrad(ws, i + 2, params, z1)
        yield from _wgrad_check(ws, i + 2, params, z1, grads_before, grads_after)
        yield from _bn_backward(ws, i + 1, params, training, S1, u * S1.abs() + tn, A1, grads_before, grads_after)
        S2, A2 = _dgrad(ws, i + 1, params, z0)
        yield from _wgrad_check(ws, i + 1, params, z0, grads_before, grads_after)
        yield from _bn_backward(ws, i, params, training, S2, u * S2.abs() + tn, A2, grads_before, grads_after)
        if ws.down[b]:
            # shortcut: batch norm without ReLU behind a pointwise (strided) convolution of the block input; its data gradient is rounded
            # to 16 bits before it joins the main branch
            yield from _bn_backward(ws, i + 3, params, training, G, R, A, grads_before, grads_after)
            T, AT = _dgrad(ws, i + 3, params, None)
            yield from _wgrad_check(ws, i + 3, params, X, grads_before, grads_after)
            skip, Rs, As = T, u * T.abs() + tn, AT
        else:
            skip, Rs, As = G, R, A
        D, AD = _dgrad(ws, i, params, None)
        yield from _wgrad_check(ws, i, params, X, grads_before, grads_after)
        # skip chain: the block-input gradient gX = gate(dgrad(dy_conv1) + skip) is the one quantity that is not a single hop.  The engine's
        # copy is one 16-bit rounding of an f32 sum whose `skip` operand is its own (rounded) gradient of the block output, so along the
        # identity chain of a layer the budget grows by one rounding (u |gX|) and one accumulation term per block passed, ADDITIVELY; a block
        # with a downsample branch restarts it, because there both operands come from stored dy tensors.
        gate = (X > 0).double() if b > 0 else torch.ones_like(X)           # the pooled stem output has no ReLU of its own
        G = (D + skip) * gate
        R = (u * G.abs() + tn + Rs) * gate
        A = (AD + As + 2 * F32_EPS * (D.abs() + skip.abs())) * gate
    # max-pool backward through the engine's own recorded taps: every input pixel sums the (<= 4) windows that chose it, one more rounding
    N, H2, W2 = ws.N, ws.H // 2, ws.W // 2
    ih, iw, ok = _pool_taps(ws)
    n_i = torch.arange(N, device=dev).view(N, 1, 1, 1).expand_as(ih)
    c_i = torch.arange(64, device=dev).view(1, 1, 1, 64).expand_as(ih)
    flat = (((n_i * H2 + ih.clamp(0, H2 - 1)) * W2 + iw.clamp(0, W2 - 1)) * 64 + c_i).reshape(-1)

    def scatter(t):
        return torch.zeros(N * H2 * W2 * 64, dtype=torch.float64, device=dev).index_add_(0, flat, t.reshape(-1)).view(N, H2, W2, 64)

    gS = scatter(G)
    RS = scatter(R) + u * gS.abs() + tn
    AS = scatter(A) + 4 * F32_EPS * scatter(G.abs())
    m = (ws.act(0, 'z').double() > 0).double()                           # the stem's own ReLU
    yield from _bn_backward(ws, 0, params, training, gS * m, RS * m, AS * m, grads_before, grads_after)
    P = ws.plan
    xpad = ws.view(P.xpad, (N, ws.H + 6, ws.W + 8, 4), ws.store).double()
    yield from _wgrad_check(ws, 0, params, xpad, grads_before, grads_after)


def evaluate(checks, verbose=True):
    """Elementwise (every element) and per-tensor (norm) verdict of a list of Check tuples: returns (failures, lines), one line per pair
    with its worst error / bound ratio."""
    worst, fails = {}, []
    for c in checks:
        got, want = c.got.double(), c.want.double()
        bound = c.bound.double().to(want.device)
        if bound.shape != want.shape:
            bound = bound.expand_as(want)
        err = (got - want).abs()
        bad_val = ~torch.isfinite(got) | ~torch.isfinite(want)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
        ratio = torch.where(bad_val, torch.full_like(ratio, float('inf')), ratio)
        r_el = float(ratio.max()) if ratio.numel() else 0.0
        nb = float(bound.norm())
        ne = float(err.norm()) if not bool(bad_val.any()) else float('inf')
        r_nm = ne / nb if nb > 0 else (0.0 if ne == 0 else float('inf'))
        rel = ne / (float(want.norm()) + 1e-300)
        w = worst.setdefault(c.pair, {})
        w[c.name] = (r_el, r_nm, rel)
        if not (r_el <= 1.0 and r_nm <= 1.0):
            k = int(ratio.reshape(-1).argmax())
            fails.append('pair %d %s: worst element error / bound %.3g (flat index %d: got %.6g want %.6g bound %.3g), norm error / bound %.3g, '
                         'relative error %.3g' % (c.pair, c.name, r_el, k, float(got.reshape(-1)[k]), float(want.reshape(-1)[k]),
                                                  float(bound.reshape(-1)[k]), r_nm, rel))
    lines = []
    for pair in sorted(worst):
        lines.append('   pair %3d  ' % pair + '  '.join('%s %.2f' % (n, v[0]) for n, v in worst[pair].items()))
    return fails, lines, worst


# ---- running the engine on a workspace the caller owns ----------------------------------------------------------------------------------
class TrunkCase:
    """A (reduced) bottleneck trunk with seeded parameters on the GPU, run through evk_trunk_forward / evk_trunk_backward by ctypes on a
    workspace between two guard bands."""

    def __init__(self, blocks, planes, N, Hh, Ww, seed=0, ill=False):
        from evoke_amd import hip as H
        self.H = H
        self.store = H.STORE_DTYPE
        cfg = H.TrunkCfg()
        for k in range(4):
            cfg.blocks[k], cfg.planes[k], cfg.stride[k] = blocks[k], planes[k], (1, 2, 2, 2)[k]
        cfg.eps, cfg.momentum = 1e-5, 0.1
        self.cfg, self.N, self.Hh, self.Ww = cfg, N, Hh, Ww
        self.nbytes = H.lib.evk_trunk_ws_bytes(C.byref(cfg), N, Hh, Ww)
        if self.nbytes < 0:
            raise RuntimeError('evk_trunk_ws_bytes: ' + H.lib.evk_last_error().decode())
        self.pairs, self.plan = H.trunk_plan(cfg, N, Hh, Ww)
        g = torch.Generator().manual_seed(seed)
        self.params, self.running0 = [], []
        for i, p in enumerate(self.pairs):
            if i == 0:
                w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5 * 2
            else:
                w = (torch.randn(p.g.Co, p.g.KH, p.g.KW, p.g.Ci, generator=g) * (2.0 / (p.g.Ci * p.g.KH * p.g.KW)) ** 0.5).to(self.store)
            gamma = 0.5 + torch.rand(p.C, generator=g)
            beta = torch.randn(p.C, generator=g) * 0.2
            if p.role == 3:
                gamma = gamma * 0.5
            if ill and p.role in (1, 2, 3) and p.C >= 16:
                # near-dead channels (|beta| >> |gamma|: the exact-sum fallback of the gate statistics), a dead one, and a channel whose
                # convolution output is constant (zero filter: variance 0, the max(., 0) clamp and invstd = 1 / sqrt(eps))
                gamma[1], beta[1] = 0.02, 1.0
                gamma[9], beta[9] = -0.01, 0.7
                gamma[3] = 0.0
                w[5] = 0
                beta[5] = 0.3
            self.params.append(dict(w=w, gamma=gamma, beta=beta))
            self.running0.append((torch.randn(p.C, generator=g) * 0.1, 0.5 + torch.rand(p.C, generator=g)))
        self.images = torch.randn(N, 3, Hh, Ww, generator=g)
        co = 4 * planes[3]
        self.dout = (torch.randn(N, Hh // 32, Ww // 32, co, generator=g) * 0.5).to(self.store)
        self.grad0 = [dict(dw=torch.randn(p_['w'].shape, generator=g) * 0.01, dgamma=torch.randn(p_['gamma'].shape, generator=g) * 0.01,
                           dbeta=torch.randn(p_['beta'].shape, generator=g) * 0.01) for p_ in self.params]

    def run(self, training, fill, side_stream=True, frozen=(), backward=True, buffer=None, on_device=False):
        """fill: the 16-bit pattern the workspace holds before the forward (0 or a NaN pattern).  frozen: {(pair, 'dw' | 'dgamma' | 'dbeta')}
        passed as NULL.  Returns dict(ws (CPU bytes), out, grads, running, guards_ok)."""
        H = self.H
        dev = 'cuda'
        big = buffer if buffer is not None else torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=dev)
        assert big.data_ptr() % 256 == 0
        big[:GUARD] = GUARD_BYTE
        big[GUARD + self.nbytes:] = GUARD_BYTE
        wsd = big[GUARD:GUARD + self.nbytes]
        wsd.view(torch.int16).fill_(fill - 65536 if fill >= 32768 else fill)
        dparams = [{k: v.to(dev).contiguous() for k, v in p.items()} for p in self.params]
        drun = [(a.to(dev), b.to(dev)) for a, b in self.running0]
        dgrads = [{k: v.to(dev).contiguous() for k, v in g.items()} for g in self.grad0]
        arr = (H.TrunkLayer * len(self.pairs))()
        for i in range(len(self.pairs)):
            l = arr[i]
            l.w, l.gamma, l.beta = dparams[i]['w'].data_ptr(), dparams[i]['gamma'].data_ptr(), dparams[i]['beta'].data_ptr()
            l.running_mean, l.running_var = drun[i][0].data_ptr(), drun[i][1].data_ptr()
            for k in ('dw', 'dgamma', 'dbeta'):
                setattr(l, k, None if (i, k) in frozen else dgrads[i][k].data_ptr())
        images, dout = self.images.to(dev), self.dout.to(dev)
        out = torch.empty_like(dout)
        n = len(self.pairs)
        torch.cuda.synchronize()
        H.check(H.lib.evk_trunk_forward(C.byref(self.cfg), arr, n, H.ptr(images), self.N, self.Hh, self.Ww, H.ptr(wsd), self.nbytes, H.ptr(out),
                                        int(training), H.stream()), 'trunk_forward')
        if backward:
            side = torch.cuda.Stream() if side_stream else None
            H.check(H.lib.evk_trunk_backward(C.byref(self.cfg), arr, n, self.N, self.Hh, self.Ww, H.ptr(wsd), self.nbytes, H.ptr(dout),
                                             int(training), H.stream(), side.cuda_stream if side is not None else None), 'trunk_backward')
            if side is not None:
                side.synchronize()
        torch.cuda.synchronize()
        guards_ok = bool((big[:GUARD] == GUARD_BYTE).all()) and bool((big[GUARD + self.nbytes:] == GUARD_BYTE).all())
        if on_device:           # (a production-size workspace is audited where it is; `big` stays alive through the view)
            grads = [{k: (None if (i, k) in frozen else v) for k, v in g.items()} for i, g in enumerate(dgrads)]
            return dict(ws=wsd, out=out, grads=grads, running=drun, guards_ok=guards_ok)
        grads = [{k: (None if (i, k) in frozen else v.cpu()) for k, v in g.items()} for i, g in enumerate(dgrads)]
        return dict(ws=wsd.cpu(), out=out.cpu(), grads=grads, running=[(a.cpu(), b.cpu()) for a, b in drun], guards_ok=guards_ok)

    def workspace(self, raw):
        ws = Workspace(raw, self.pairs, self.plan, self.store)
        ws.N, ws.H, ws.W = self.N, self.Hh, self.Ww
        return ws

    def calibrate(self):
        """Running statistics := the batch statistics of these images (one train-mode forward with momentum 1).  A deep trunk with random
        weights and unrelated running statistics leaves fp16's range in eval mode within a few blocks; the eval-mode audit of the deep cases
        starts from statistics a trained network would have."""
        self.cfg.momentum = 1.0
        try:
            self.running0 = self.run(True, 0, backward=False)['running']
        finally:
            self.cfg.momentum = 0.1

    def audit(self, res, training, frozen=(), backward=True):
        """generator of Check tuples (evaluate() consumes it one hop at a time: a full-size trunk's tensors are not all kept)"""
        ws = self.workspace(res['ws'])
        yield from audit_forward(ws, self.params, self.images, training, 1e-5, 0.1, self.running0, res['running'], res['out'])
        if backward:
            before = [{k: (None if (i, k) in frozen else v) for k, v in g.items()} for i, g in enumerate(self.grad0)]
            yield from audit_backward(ws, self.params, self.dout, training, before, res['grads'])


# ---- a plain fp32 CPU evaluation of the same hops, stored the way the engine stores them ------------------------------------------------
def emulate_engine(case, training, mutate=None):
    """The runner's arithmetic restated with torch on the CPU: f32 products and sums, 16-bit roundings where the engine stores 16 bits, the
    workspace filled in at the offsets of evk_trunk_plan.  It is what the derived bounds are checked against without a GPU (the audit must
    accept it and must reject the `mutate`d variants: tests/test_trunk_audit_cpu.py), and the "fp32 evaluation of the same hop" of the
    bounds' derivation.  mutate: None, or one defect -- 'sum_gx' (x 1.02 in every pair), 'bessel' (running variance without n / (n - 1)),
    'stats_row' (the last row missing from the forward statistics), 'gate' (a data gradient gated with >= 0 instead of > 0)."""
    st_t, f32 = case.store, torch.float32
    raw = torch.zeros(case.nbytes, dtype=torch.uint8)
    ws = case.workspace(raw)
    P, N, H, W = case.plan, case.N, case.Hh, case.Ww
    eps, mom = 1e-5, 0.1

    def put(off, t):
        b = t.contiguous().view(-1).view(torch.uint8)
        raw[off:off + b.numel()].copy_(b)

    xpad = torch.zeros(N, H + 6, W + 8, 4, dtype=st_t)
    xpad[:, 3:H + 3, 3:W + 3, :3] = case.images.permute(0, 2, 3, 1).to(st_t)
    wp = torch.zeros(64, 7, 8, 4, dtype=st_t)
    wp[:, :, :7, :3] = case.params[0]['w'].permute(0, 2, 3, 1).to(st_t)
    put(P.xpad, xpad)
    put(P.wp, wp)
    running = [(a.clone(), b.clone()) for a, b in case.running0]
    Y, Z, ST = {}, {}, {}
    pooled = None

    def block_input(b):
        return pooled if b == 0 else Z[ws.first[b - 1] + 2]

    order = [0]
    for b, i in enumerate(ws.first):
        order += ([i + 3] if ws.down[b] else []) + [i, i + 1, i + 2]
    for i in order:
        p = case.pairs[i]
        gamma, beta = case.params[i]['gamma'], case.params[i]['beta']
        idt, relu = None, p.role != 4
        if i == 0:
            conv = conv64(xpad.float(), wp.float(), 2, 0)[:, :, :W // 2].contiguous()
        else:
            xin = block_input(p.block) if p.role in (1, 4) else Z[i - 1]
            conv = conv64(xin.float(), case.params[i]['w'].float(), p.g.stride_h, p.g.pad_h)
            if p.role == 3:
                idt = (Z[i + 1] if ws.down[p.block] else block_input(p.block)).float()
        M = float(p.M)
        y = conv.to(st_t)
        st = torch.zeros(6, p.C, dtype=f32)
        if training:
            c2 = conv.reshape(-1, p.C)
            if mutate == 'stats_row':
                c2 = c2[:-1]
            st[0], st[1] = c2.sum(0), (c2 * c2).sum(0)
            mean = st[0] / M
            var = (st[1] / M - mean * mean).clamp_min(0)
            rm, rv = running[i]
            bess = 1.0 if mutate == 'bessel' else M / max(M - 1.0, 1.0)
            running[i] = ((1 - mom) * rm + mom * mean, (1 - mom) * rv + mom * var * bess)
        else:
            mean, var = running[i]
        istd = (var + eps).rsqrt()
        st[2], st[3], st[4], st[5] = gamma * istd, beta - mean * gamma * istd, mean, istd
        z = y.float() * st[2] + st[3]
        if idt is not None:
            z = z + idt
        z = (z.clamp_min(0) if relu else z).to(st_t)
        Y[i], Z[i], ST[i] = y, z, st
        put(p.y, y)
        put(p.z, z)
        put(p.stats, st)
        if i == 0:
            mp, ind = F.max_pool2d(_nchw(z.float()), 3, 2, 1, return_indices=True)
            pooled = mp.permute(0, 2, 3, 1).to(st_t).contiguous()
            ind = ind.permute(0, 2, 3, 1)
            ih, iw = ind // (W // 2), ind % (W // 2)
            oh = torch.arange(H // 4).view(1, -1, 1, 1)
            ow = torch.arange(W // 4).view(1, 1, -1, 1)
            taps = ((ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))).to(torch.uint8)
            put(P.pooled, pooled)
            put(P.pool_idx, taps)
    last = ws.first[-1] + 2
    out = Z[last].clone()
    grads = [{k: v.clone() for k, v in g.items()} for g in case.grad0]

    def bn_bwd(i, dz):
        p, st = case.pairs[i], ST[i]
        M = float(p.M)
        g, yv = dz.float(), Y[i].float()
        xhat = (yv - st[4]) * st[5]
        sg, sgx = g.reshape(-1, p.C).sum(0), (g * xhat).reshape(-1, p.C).sum(0)
        if mutate == 'sum_gx':
            sgx = sgx * 1.02
        put(p.sums, torch.stack([sg, sgx]))
        grads[i]['dbeta'] += sg
        grads[i]['dgamma'] += sgx
        dy = st[2] * (g - sg / M - xhat * (sgx / M)) if training else st[2] * g
        dy = dy.to(st_t)
        put(p.dy, dy)
        return dy

    def dgrad(i, dy):
        g = case.pairs[i].g
        return dgrad64(dy.float(), case.params[i]['w'].float(), (g.N, g.Hi, g.Wi, g.Ci), g.stride_h, g.pad_h)

    def wgrad(i, dy, xin):
        g = case.pairs[i].g
        grads[i]['dw'] += wgrad64(dy.float(), xin.float(), (g.Co, g.KH, g.KW, g.Ci), g.stride_h, g.pad_h)

    G = (case.dout.float() * (Z[last].float() > 0)).to(st_t)
    for b in range(len(ws.first) - 1, -1, -1):
        i = ws.first[b]
        X = block_input(b)
        dy3 = bn_bwd(i + 2, G)
        gate1 = Z[i + 1].float() >= 0 if mutate == 'gate' else Z[i + 1].float() > 0
        S1 = (dgrad(i + 2, dy3) * gate1).to(st_t)
        wgrad(i + 2, dy3, Z[i + 1])
        dy2 = bn_bwd(i + 1, S1)
        S2 = (dgrad(i + 1, dy2) * (Z[i].float() > 0)).to(st_t)
        wgrad(i + 1, dy2, Z[i])
        dy1 = bn_bwd(i, S2)
        skip = G.float()
        if ws.down[b]:
            dyd = bn_bwd(i + 3, G)
            skip = dgrad(i + 3, dyd).to(st_t).float()
            wgrad(i + 3, dyd, X)
        gx = dgrad(i, dy1) + skip
        if b > 0:
            gx = gx * (X.float() > 0)
        wgrad(i, dy1, X)
        G = gx.to(st_t)
    ih, iw, _ = _pool_taps(ws)
    n_i = torch.arange(N).view(N, 1, 1, 1).expand_as(ih)
    c_i = torch.arange(64).view(1, 1, 1, 64).expand_as(ih)
    flat = (((n_i * (H // 2) + ih) * (W // 2) + iw) * 64 + c_i).reshape(-1)
    gS = torch.zeros(N * (H // 2) * (W // 2) * 64, dtype=f32).index_add_(0, flat, G.float().reshape(-1)).view(N, H // 2, W // 2, 64).to(st_t)
    dy0 = bn_bwd(0, (gS.float() * (Z[0].float() > 0)).to(st_t))
    dwp = wgrad64(F.pad(dy0.float(), (0, 0, 0, 1)), xpad.float(), (64, 7, 8, 4), 2, 0)
    grads[0]['dw'] += dwp[:, :, :7, :3].permute(0, 3, 1, 2)
    return dict(ws=raw, out=out, grads=grads, running=running, guards_ok=True)
