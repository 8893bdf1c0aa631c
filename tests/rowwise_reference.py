"""float64 restatements of the row-wise and element-wise kernels (csrc/norm.hip, csrc/eltwise.hip) and the error model of the tests that
compare the kernels with them (tests/test_rowwise_edges_gpu.py).  Plain torch on the CPU; tests/test_rowwise_reference_cpu.py pins the
restatements to torch's own operators.

Error model (the bounds come from the number formats, never from a kernel's output):
  * f32 outputs: the project's bound 1e-5 + 1e-5 |want| (f32_tol), plus 4 spacing_f32(max |input| of the row) where the inputs carry a
    large offset -- the f32 INPUT grid is that coarse, and a difference of two inputs cannot be known better.
  * 16-bit outputs of f32 arithmetic WITHOUT a subtraction of nearly equal quantities (softmax probabilities, dropout scaling,
    activations, casts): one unit in the last place of the storage format at the float64 value (ulp16), subnormal spacing at the bottom.
  * 16-bit outputs of f32 arithmetic WITH such a subtraction: one ulp16 cannot hold where the operands cancel, because the f32 result carries
    the rounding of its OPERANDS whatever the size of the difference.  Measured against one ulp alone (fp16 / bf16 build): LayerNorm y 1.8e3 /
    1.1e4 ulp (rows at offset 1000), LayerNorm dx and ddgam 2.5 / 290, dlogits = softmax - onehot 4.0 (fp16), GELU' 0.9 / 216 and GELU_NEW'
    13.5 / 256 at their zero crossing.  For these the bound is ulp16(want) plus a few 2^-24 times the operand magnitudes of the float64
    reference, derived per kernel in tests/test_rowwise_edges_gpu.py; where nothing cancels that term is a small fraction of one ulp, so
    the check keeps the issue's strength there.  Softmax dS measured 0.5 ulp on real data and stays at one ulp.
"""
import math

import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------ number formats
def fmt(dtype):
    """(significand bits with the hidden one, exponent of the smallest normal, exponent of the largest binade)"""
    return {torch.float16: (11, -14, 15), torch.bfloat16: (8, -126, 127), torch.float32: (24, -126, 127)}[dtype]


def ulp(x, dtype):
    """spacing of `dtype` at the float64 value(s) x: 2^(e - p + 1) with e = floor(log2 |x|) clamped to the normal range (so a power of two
    gets the spacing ABOVE it, and everything below the smallest normal the subnormal spacing)"""
    p, emin, emax = fmt(dtype)
    x = torch.as_tensor(x, dtype=F64).abs()
    _, e = torch.frexp(torch.where(torch.isfinite(x) & (x > 0), x, torch.ones_like(x)))      # x = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp(emin, emax).to(F64)
    e = torch.where(x > 0, e, torch.full_like(e, emin))
    return torch.exp2(e - (p - 1))


def spacing_f32(x):
    return float(ulp(torch.tensor(float(x), dtype=F64), torch.float32))


def f32_tol(want, extra=0.0):
    return 1e-5 + 1e-5 * want.abs() + extra


def all_patterns(dtype):
    """every 16-bit pattern as a tensor of `dtype` (index = pattern)"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def finite_values(dtype):
    v = all_patterns(dtype)
    return v[torch.isfinite(v.float())]


def rne_probes(dtype):
    """f32 inputs that decide round-to-nearest-even into `dtype`: every finite value, the exact midpoint of every pair of neighbours (a tie:
    must go to the even neighbour), one f32 step either side of every midpoint, and past the largest finite value the midpoint to the
    next power of two (a tie that rounds to inf), one f32 step towards zero and one away from it, and the largest f32 (both signs)."""
    v = torch.unique(finite_values(dtype).to(F64))             # sorted, -0 == +0 merged
    mid = (v[:-1] + v[1:]) / 2                                    # one more significand bit than `dtype`: exact in f32
    mid32 = mid.to(torch.float32)
    assert bool((mid32.to(F64) == mid).all())
    inf = torch.tensor(float('inf'))
    top = float(v[-1]) + float(ulp(v[-1], dtype)) / 2
    top32 = torch.tensor([top, -top], dtype=torch.float32)
    parts = [v.to(torch.float32), mid32, torch.nextafter(mid32, -inf), torch.nextafter(mid32, inf),
             top32, torch.nextafter(top32, torch.zeros(2)), torch.nextafter(top32, torch.sign(top32) * inf), torch.tensor([3.4028234663852886e38, -3.4028234663852886e38])]
    return torch.cat(parts)


def cast_specials():
    """+-0, +-inf, NaN, f32 subnormals (smallest, largest, one in between) and their negatives"""
    sub = torch.tensor([1, 0x7fffff, 0x400000, 0x12345], dtype=torch.int32).view(torch.float32)
    return torch.cat([torch.tensor([0.0, -0.0, float('inf'), -float('inf'), float('nan')]), sub, -sub])


# ------------------------------------------------------------------------------------------------------------ softmax
def attend(B, heads, Tq, S, mask=None, causal=False):
    """bool [B, heads, Tq, S]: which entries take part (mask uint8 [B, S] or [B, Tq, S], 1 = attend; causal: col <= q)"""
    on = torch.ones(B, heads, Tq, S, dtype=torch.bool)
    if mask is not None:
        on &= (mask[:, None, None, :] if mask.dim() == 2 else mask[:, None, :, :]).bool()
    if causal:
        on &= torch.arange(S)[None, :] <= torch.arange(Tq)[:, None]
    return on


def masked_softmax(scores, on):
    """float64 softmax over the last dim of the entries `on`; an entry that is off or -inf gets 0, a row without any entry is all 0"""
    s = scores.to(F64).masked_fill(~on, -float('inf'))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    return torch.where(z > 0, e / z, torch.zeros_like(e))


def softmax_bwd(P, dP, alpha):
    P, dP = P.to(F64), dP.to(F64)
    return alpha * P * (dP - (dP * P).sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm(x, gamma, beta, eps, mode, dgam=None, dbet=None):
    """mode 0: torch.nn.LayerNorm (biased variance, eps inside the root); mode 1: g (x - mu) / (unbiased std + eps) + b.  Per-row deltas
    dgam / dbet are added to gamma / beta.  Returns (y, mean, rstd, xhat)."""
    x = x.to(F64)
    g = gamma.to(F64) + (dgam.to(F64) if dgam is not None else 0)
    b = beta.to(F64) + (dbet.to(F64) if dbet is not None else 0)
    mu = x.mean(-1, keepdim=True)
    q = ((x - mu) ** 2).sum(-1, keepdim=True)
    D = x.shape[-1]
    r = 1 / torch.sqrt(q / D + eps) if mode == 0 else 1 / (torch.sqrt(q / (D - 1)) + eps)
    xh = (x - mu) * r
    return xh * g + b, mu[..., 0], r[..., 0], xh


# ------------------------------------------------------------------------------------------------------------ log-softmax
def log_softmax(x, scale=1.0):
    """float64; -inf entries stay -inf (never NaN) as long as the row has a finite entry"""
    x = x.to(F64) * scale
    m = x.max(-1, keepdim=True).values
    lse = m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))
    return x - lse, lse[..., 0]


# ------------------------------------------------------------------------------------------------------------ activations
ACTS = dict(relu=1, gelu=2, tanh=3, sigmoid=4, gelu_new=5)          # evoke_amd.hip ACT_*
K0, K1 = math.sqrt(2 / math.pi), 0.044715


def _sigmoid(x):
    e = torch.exp(-x.abs())                                      # no overflow, no cancellation on either side
    return torch.where(x >= 0, 1 / (1 + e), e / (1 + e))


def act(x, name):
    """float64 activation, accurate in the tails: 1 + erf(x / sqrt 2) and 1 + tanh(u) cancel for x << 0, erfc and the logistic form do not"""
    x = x.to(F64)
    if name == 'relu':
        return x.clamp_min(0)
    if name == 'gelu':
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2))
    if name == 'tanh':
        return torch.tanh(x)
    if name == 'sigmoid':
        return _sigmoid(x)
    if name == 'gelu_new':
        return x * _sigmoid(2 * K0 * (x + K1 * x ** 3))         # 0.5 (1 + tanh u) == logistic(2 u)
    raise ValueError(name)


def act_grad(ref, name):
    """float64 d act / d x as the kernel's backward sees it: as a function of the OUTPUT for relu / tanh / sigmoid, of the pre-activation
    for the two GELUs"""
    r = ref.to(F64)
    if name == 'relu':
        return (r > 0).to(F64)
    if name == 'tanh':
        return 1 - r * r
    if name == 'sigmoid':
        return r * (1 - r)
    if name == 'gelu':
        return 0.5 * torch.special.erfc(-r / math.sqrt(2)) + r * torch.exp(-0.5 * r * r) / math.sqrt(2 * math.pi)
    if name == 'gelu_new':
        u = K0 * (r + K1 * r ** 3)
        s = _sigmoid(2 * u)
        rr = torch.where(torch.isfinite(r * r), r * r, torch.zeros_like(r))
        return s + r * 2 * s * (1 - s) * K0 * (1 + 3 * K1 * rr)           # d/dx [x s(2u)], s' = s (1 - s)
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------------------ top-k
def topk_rows(x, k):
    """the k largest of every row in descending order, ties -> lowest index first: a STABLE descending sort"""
    v, i = torch.sort(x.to(F64), dim=-1, descending=True, stable=True)
    return v[..., :k], i[..., :k]


# ------------------------------------------------------------------------------------------------------------ L2 norm, soft cross-entropy
def l2norm(x, eps=1e-12):
    x = x.to(F64)
    n = x.norm(dim=-1, keepdim=True).clamp_min(eps)
    return x / n, n[..., 0]


def softce(z, t, scale, diag_mask):
    """(sum over rows of -sum_c t log_softmax(z)) * scale with z[r][r] = -1e9 under diag_mask; returns the loss and the z it was taken of"""
    z = z.to(F64).clone()
    if diag_mask:
        idx = torch.arange(min(z.shape))
        z[idx, idx] = -1e9
    lp, _ = log_softmax(z)
    return -(t.to(F64) * lp).sum() * scale, z
