"""Float64 restatement of what evk_decode_attention_maps emits: for query row r the head mean of the masked softmax over the keys,

    maps[r, s] = (1 / H) * sum_h softmax_s(scale * q[r, h] . K[r // kv_div, s, h])        (MultiHeadedAttention.attn averaged over heads,
                                                                                          modules/encoder_decoder.py:189,200)

computed from the 16-bit operands widened to float64, with the error bound the GPU test holds the f32 kernel to.  The bound is derived from
the operands, not fitted (u = 2^-24, the unit roundoff of f32):

    per head   p64 * u * (128 * A + 2 * (|x_s| + 2) + S + 2)
        A = scale * max_s sum_i |q_i k_si|: the operand magnitude of a 64-term f32 dot product (64 u per product sum), counted twice -- the
            score itself and the row maximum it is measured from both carry it into the exponent;
        x_s = scaled score minus the row maximum, the exponent's argument: one rounding of the scaling multiply (base-2 exponential) on an
            argument of size |x_s|, plus the exponential instruction's own error;
        S + 2: the sum of S terms and the division.
    head mean  the per-head bounds averaged, plus 8 u of the mean for the sum over the heads and the multiplication by 1 / H.
    floor      2^-100 absolute: what the hardware flushes to zero is below it.
Masked keys are exactly 0 and carry no bound; a row whose keys are all masked is a row of zeros.
"""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -100


def head_mean_softmax(q, k, mask, scale, kv_div=1):
    """q (R, H, dh), k (R // kv_div, S, H, dh) -- values of 16-bit operands, any float dtype --, mask (R // kv_div, S) of 0 / 1 or None
    -> dict: maps (R, S) f64, bound (R, S) f64, heads (R, H, S) f64 the per-head probabilities"""
    q = np.asarray(q, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    R, H, _ = q.shape
    S = k.shape[1]
    rk = np.arange(R) // kv_div
    kk = k[rk]                                                        # (R, S, H, dh)
    x = scale * np.einsum('rhd,rshd->rhs', q, kk)
    A = scale * np.einsum('rhd,rshd->rhs', np.abs(q), np.abs(kk)).max(-1)          # (R, H)
    keep = np.ones((R, S), dtype=bool) if mask is None else np.asarray(mask)[rk].astype(bool)
    x = np.where(keep[:, None, :], x, -np.inf)
    m = x.max(-1, keepdims=True)
    live = np.isfinite(m)
    xs = np.where(keep[:, None, :] & live, x - np.where(live, m, 0.0), -np.inf)     # exponent's argument, -inf where masked
    e = np.exp(xs)
    den = e.sum(-1, keepdims=True)
    p = np.where(den > 0, e / np.where(den > 0, den, 1.0), 0.0)
    ax = np.where(np.isfinite(xs), np.abs(xs), 0.0)
    per_head = p * U * (128.0 * A[..., None] + 2.0 * (ax + 2.0) + S + 2.0)
    maps = p.sum(1) / H
    bound = per_head.mean(1) + 8.0 * U * maps + FLOOR
    return dict(maps=maps, bound=bound, heads=p)
