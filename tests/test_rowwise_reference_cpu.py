"""CPU checks of tests/rowwise_reference.py, the float64 restatements the GPU edge tests of the row-wise and element-wise kernels compare
with (tests/test_rowwise_edges_gpu.py): each restatement against torch's own operator, and the helpers of the error model against
hand-computed values."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import rowwise_reference as R

F64 = torch.float64


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize('D', [8, 520])
def test_layernorm_restatement_mode0_is_torch_layer_norm(D):
    x, g, b = rnd(5, D, seed=1) * 3 + 2, 1 + 0.2 * rnd(D, seed=2), rnd(D, seed=3)
    y, mu, r, xh = R.layernorm(x, g, b, 1e-5, 0)
    assert float((y - F.layer_norm(x, (D,), g, b, 1e-5)).abs().max()) < 1e-13
    assert float((mu - x.mean(-1)).abs().max()) < 1e-14 and float((r - 1 / torch.sqrt(x.var(-1, unbiased=False) + 1e-5)).abs().max()) < 1e-13
    # mode 1 with per-row deltas: the formula of the reference's ConditionalLayerNorm, written out independently
    dg, db = 0.3 * rnd(5, D, seed=4), 0.3 * rnd(5, D, seed=5)
    y1 = R.layernorm(x, g, b, 1e-6, 1, dg, db)[0]
    want = (g + dg) * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + 1e-6) + (b + db)
    assert float((y1 - want).abs().max()) < 1e-13


def test_activation_restatements_match_torch_where_torch_is_accurate():
    x = torch.linspace(-6, 6, 2401, dtype=F64)
    assert float((R.act(x, 'gelu_new') - F.gelu(x, approximate='tanh')).abs().max()) < 1e-15
    assert float((R.act(x, 'gelu') - F.gelu(x)).abs().max()) < 1e-15
    assert float((R.act(x, 'sigmoid') - torch.sigmoid(x)).abs().max()) < 1e-15
    assert float((R.act(x, 'tanh') - torch.tanh(x)).abs().max()) == 0 and float((R.act(x, 'relu') - F.relu(x)).abs().max()) == 0
    # the tails, where 1 + erf and 1 + tanh cancel: against the asymptotic forms, to a relative 1e-3
    assert abs(float(R.act(torch.tensor(-10.0, dtype=F64), 'gelu')) / (-10 * 0.5 * math.erfc(10 / math.sqrt(2))) - 1) < 1e-12
    u = R.K0 * (-8 + R.K1 * -512)
    assert abs(float(R.act(torch.tensor(-8.0, dtype=F64), 'gelu_new')) / (-8 * math.exp(2 * u)) - 1) < 1e-3
    assert float(R.act(torch.tensor(-3e38, dtype=F64), 'gelu_new')) == 0 and float(R.act(torch.tensor(3e38, dtype=F64), 'gelu_new')) == 3e38
    # derivatives against autograd of torch's operators
    for name, fn in (('gelu', F.gelu), ('gelu_new', lambda t: F.gelu(t, approximate='tanh')), ('tanh', torch.tanh), ('sigmoid', torch.sigmoid),
                     ('relu', F.relu)):
        xs = torch.linspace(-5, 5, 1001, dtype=F64).requires_grad_(True)
        y = fn(xs)
        y.sum().backward()
        ref = xs.detach() if name.startswith('gelu') else y.detach()
        assert float((R.act_grad(ref, name) - xs.grad).abs().max()) < 1e-14, name


def test_ulp_helper_at_normal_subnormal_and_power_of_two_values():
    h, b = torch.float16, torch.bfloat16
    assert float(R.ulp(1.0, h)) == 2.0 ** -10 and float(R.ulp(1.5, h)) == 2.0 ** -10 and float(R.ulp(1.999, h)) == 2.0 ** -10
    assert float(R.ulp(2.0, h)) == 2.0 ** -9 and float(R.ulp(-2.0, h)) == 2.0 ** -9 and float(R.ulp(0.999, h)) == 2.0 ** -11
    assert float(R.ulp(2.0 ** -14, h)) == 2.0 ** -24 and float(R.ulp(2.0 ** -15, h)) == 2.0 ** -24 and float(R.ulp(0.0, h)) == 2.0 ** -24
    assert float(R.ulp(1e-30, h)) == 2.0 ** -24 and float(R.ulp(65504.0, h)) == 32.0 and float(R.ulp(1e9, h)) == 32.0
    assert float(R.ulp(1.0, b)) == 2.0 ** -7 and float(R.ulp(2.0 ** -126, b)) == 2.0 ** -133 and float(R.ulp(1e-40, b)) == 2.0 ** -133
    assert float(R.ulp(3.0, b)) == 2.0 ** -6 and R.spacing_f32(30000.0) == 2.0 ** -9 and R.spacing_f32(1.0) == 2.0 ** -23
    # against the formats themselves: the distance from every positive finite value to the next one
    for dt in (h, b):
        v = torch.unique(R.finite_values(dt).to(F64))
        v = v[v >= 0]
        assert bool((R.ulp(v[:-1], dt) == v[1:] - v[:-1]).all())


@pytest.mark.parametrize('dt', [torch.float16, torch.bfloat16])
def test_rne_probes_hold_exact_midpoints_and_their_f32_neighbours(dt):
    p = R.rne_probes(dt)
    assert p.dtype == torch.float32 and bool(torch.isfinite(p).all())
    v = torch.unique(R.finite_values(dt).to(F64))
    n = len(v)
    mid = p[n:2 * n - 1].to(F64)
    assert bool((mid - v[:-1] == v[1:] - mid).all()), 'a midpoint probe is not the exact midpoint'
    # torch's own conversion sends every tie to the neighbour with the even pattern, and the f32 steps either side to the nearer one
    got = mid.to(torch.float32).to(dt)
    assert bool(((got.view(torch.int16).to(torch.int32) & 1) == 0).all())
    lo, hi = p[2 * n - 1:3 * n - 2], p[3 * n - 2:4 * n - 3]
    assert bool((lo.to(F64) < mid).all()) and bool((hi.to(F64) > mid).all())
    assert bool((lo.to(dt).to(F64) == v[:-1]).all()) and bool((hi.to(dt).to(F64) == v[1:]).all())
    # past the largest finite value: the tie and everything above it become inf, one f32 step below it stays finite
    top = p[4 * n - 3:]
    t16 = top.to(dt).float()
    assert torch.isinf(t16[0]) and torch.isinf(t16[1]) and torch.isfinite(t16[2]) and torch.isfinite(t16[3]) and bool(torch.isinf(t16[4:]).all())


def test_topk_restatement_breaks_ties_towards_the_lowest_index():
    x = torch.tensor([[1.0, 3.0, 3.0, -float('inf'), 3.0, 2.0, float('inf'), 2.0], [0.0] * 8])
    v, i = R.topk_rows(x, 5)
    assert i.tolist() == [[6, 1, 2, 4, 5], [0, 1, 2, 3, 4]] and v[0].tolist() == [float('inf'), 3.0, 3.0, 3.0, 2.0]
    v, i = R.topk_rows(torch.full((1, 6), -float('inf')), 3)
    assert i.tolist() == [[0, 1, 2]]


def test_masked_softmax_log_softmax_l2norm_and_softce_restatements():
    s = rnd(2, 3, 4, 9, seed=1)
    mask = (torch.rand(2, 4, 9, generator=torch.Generator().manual_seed(2)) > 0.4).to(torch.uint8)
    mask[1, 2] = 0                                                    # a row without any key
    on = R.attend(2, 3, 4, 9, mask, causal=True)
    assert not bool(on[1, :, 2].any()) and bool(on[0, 0, 3, :4].eq(mask[0, 3, :4].bool()).all()) and not bool(on[:, :, 0, 1:].any())
    P = R.masked_softmax(s, on)
    want = torch.softmax(s.masked_fill(~on, -1e300), -1) * on
    assert float((P - want)[on.any(-1)].abs().max()) < 1e-15 and float(P[1, :, 2].abs().max()) == 0 and not bool(torch.isnan(P).any())
    Pa = torch.softmax(s, -1).requires_grad_(True)
    dP = rnd(2, 3, 4, 9, seed=3)
    sa = s.clone().requires_grad_(True)
    (torch.softmax(sa * 0.5, -1) * dP).sum().backward()
    assert float((R.softmax_bwd(torch.softmax(s * 0.5, -1), dP, 0.5) - sa.grad).abs().max()) < 1e-15
    x = rnd(4, 11, seed=4)
    x[0, 3] = -float('inf')
    lp, lse = R.log_softmax(x)
    assert float((lp - F.log_softmax(x, -1)).abs()[torch.isfinite(lp)].max()) < 1e-14 and lp[0, 3] == -float('inf') and not bool(torch.isnan(lp).any())
    z = rnd(3, 7, seed=5)
    z[1] = 0
    assert float((R.l2norm(z)[0] - F.normalize(z, dim=-1, eps=1e-12)).abs().max()) < 1e-15
    zz, t = rnd(5, 5, seed=6), torch.softmax(rnd(5, 5, seed=7), -1)
    assert abs(float(R.softce(zz, t, 0.2, False)[0]) - float(F.cross_entropy(zz, t))) < 1e-14
    t0 = t.clone()
    t0.fill_diagonal_(0)
    assert abs(float(R.softce(zz, t0, 0.2, True)[0]) - float(F.cross_entropy(zz.clone().fill_diagonal_(-1e9), t0))) < 1e-9
