"""The NumPy model of pd_per_sample (include/pdenv.h) on top of philox_np: keys, selection, weights
(test helper).  Everything in binary64, as the header states it."""
import numpy as np

from philox_np import philox, u01

TAG_PER = 48
ULP64 = 2.0 ** -52
KEY_BOUND = 32 * ULP64      # the key check's bound against this model (7.1e-15 relative)


def uniforms(size, seed, draw):
    """u_i in (0, 1]: Philox block m = i >> 1, counter (m, draw lo, draw hi, 48), key = the seed's
    halves; the even item takes 1 - u01(x, y), the odd one 1 - u01(z, w)."""
    m = np.arange((size + 1) // 2, dtype=np.uint64)
    x, y, z, w = philox(m, draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, TAG_PER, seed & 0xFFFFFFFF,
                        (seed >> 32) & 0xFFFFFFFF)
    u = np.empty(2 * m.size, dtype=np.float64)
    u[0::2] = 1.0 - u01(x, y)
    u[1::2] = 1.0 - u01(z, w)
    return u[:size]


def item_weights(priorities, alpha):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(priorities, dtype=np.float32).astype(np.float64), float(alpha))


def keys(priorities, alpha, seed, draw):
    """e_i = -log(u_i) / w_i, +inf unless 0 < w_i < inf."""
    w = item_weights(priorities, alpha)
    u = uniforms(w.size, seed, draw)
    ok = (w > 0) & (w < np.inf)
    e = np.full(w.size, np.inf)
    with np.errstate(all="ignore"):
        e[ok] = -np.log(u[ok]) / w[ok] + 0.0
    return e


def select(e, batch):
    """The batch smallest keys, ascending, ties to the lower index; -1 past the finite keys."""
    order = np.argsort(e, kind="stable")[:batch]
    idx = np.full(batch, -1, dtype=np.int64)
    n = min(batch, int(np.isfinite(e).sum()))
    idx[:n] = order[:n]
    return idx, n


def importance(priorities, alpha, beta, idx):
    """float32((size w_j / sum w)^-beta / max over the batch), the formula of sac_pytorch.py:104-108
    in binary64 (the sum over the items that take part); 0 where idx is -1."""
    w = item_weights(priorities, alpha)
    ok = (w > 0) & (w < np.inf)
    total = w[ok].sum()
    out = np.zeros(idx.size, dtype=np.float64)
    sel = idx >= 0
    if sel.any():
        v = (w.size * w[idx[sel]] / total) ** (-float(beta))
        out[sel] = v / v.max()
    return out.astype(np.float32)


def sample(priorities, batch, alpha, beta, seed, draw):
    """(indices, weights, keys, slots filled, finite keys)."""
    e = keys(priorities, alpha, seed, draw)
    idx, n = select(e, batch)
    return idx, importance(priorities, alpha, beta, idx), e, n, int(np.isfinite(e).sum())


def min_gap(e, batch):
    """The smallest relative gap between neighbours among the first batch + 1 sorted finite keys."""
    s = np.sort(e[np.isfinite(e)])[:batch + 1]
    if s.size < 2:
        return np.inf
    return float(np.min(np.diff(s) / s[1:]))
