"""NumPy binary64 model of pd_sac_learning_stats' 37 columns (include/pdenv.h), from float32 inputs:
the model of the GPU tests and the yardstick the reference's own float32 values are held against.
Not a test."""
import numpy as np

NAMES = ["step",
         "state_mean", "state_min", "state_max", "state_std", "state_kurtosis",
         "action_mean", "action_min", "action_max", "action_std", "action_kurtosis",
         "reward_mean", "reward_min", "reward_max", "reward_std", "reward_kurtosis",
         "critic_loss", "actor_loss", "alpha_loss", "alpha_value",
         "q_value_mean", "q_value_min", "q_value_max", "q_value_std",
         "log_prob_mean", "log_prob_min", "log_prob_max", "log_prob_std",
         "target_q_mean", "target_q_min", "target_q_max", "target_q_std",
         "per_beta", "per_mean_weight", "per_max_priority",
         "actor_grad_norm", "critic_grad_norm"]
N_STATS = 37
KINDS = ("mean", "min", "max", "std", "kurtosis")


def series_stats(x):
    """(mean, min, max, std ddof 0, kurtosis Fisher biased) of a flat float32 series in binary64,
    two-pass; a NaN anywhere makes all five NaN; m2 == 0 gives kurtosis 0 / 0 = NaN."""
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(np.float64)
    n = x.size
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = x.sum() / n
        d2 = (x - mean) ** 2
        m2, m4 = d2.sum() / n, (d2 * d2).sum() / n
        out = np.array([mean, x.min(), x.max(), np.sqrt(m2), m4 / (m2 * m2) - 3.0])
    if np.isnan(x).any():
        out[:] = np.nan
    return out


def series_scale(x):
    """The scale an error of each of the five statistics is relative to: max|x| for mean, min, max
    and std, kurtosis + 3 for the kurtosis."""
    st = series_stats(x)
    m = np.abs(np.asarray(x, dtype=np.float64)).max()
    return np.array([m, m, m, m, st[4] + 3.0])


def _scalar(v):
    return np.nan if v is None else float(np.asarray(v, dtype=np.float32).reshape(-1)[0])


def series_of(rows, q, target_q, log_prob, state_dim, action_dim):
    """The series, keyed by column prefix ("state" holds one per dimension)."""
    S, A = state_dim, action_dim
    rows = np.asarray(rows, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32).reshape(-1, 2)
    return {"state": [rows[:, d] for d in range(S)], "action": rows[:, S:S + A].reshape(-1), "reward": rows[:, S + A],
            "q_value": np.fmin(q[:, 0], q[:, 1]), "log_prob": np.asarray(log_prob, dtype=np.float32).reshape(-1),
            "target_q": np.asarray(target_q, dtype=np.float32).reshape(-1)}


def model_row(rows, q, target_q, log_prob, state_dim, action_dim, weights=None, critic_loss=None, actor_loss=None,
              alpha_loss=None, log_alpha=0.0, max_priority=None, actor_grad_norm=None, critic_grad_norm=None,
              per_beta=float("nan"), step=0, scales=False):
    """The [37] binary64 row; scales=True: also the [37] scale of each column's error bound (1 for the
    copied columns, which must be equal)."""
    ser = series_of(rows, q, target_q, log_prob, state_dim, action_dim)
    out, sc = np.full(N_STATS, np.nan), np.ones(N_STATS)
    out[0] = float(step)
    per_dim = np.array([series_stats(x) for x in ser["state"]])
    out[1:6] = per_dim.sum(0) / state_dim
    sc[1:6] = np.array([series_scale(x) for x in ser["state"]]).sum(0) / state_dim
    for name, col, k in (("action", 6, 5), ("reward", 11, 5), ("q_value", 20, 4), ("log_prob", 24, 4), ("target_q", 28, 4)):
        out[col:col + k] = series_stats(ser[name])[:k]
        sc[col:col + k] = series_scale(ser[name])[:k]
    out[16], out[17], out[18] = _scalar(critic_loss), _scalar(actor_loss), _scalar(alpha_loss)
    out[19] = np.exp(np.float64(_scalar(log_alpha)))
    sc[19] = out[19]
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32).reshape(-1)
        out[32], out[33] = per_beta, series_stats(w)[0]
        sc[33] = np.abs(w).max()
    out[34] = _scalar(max_priority)
    out[35], out[36] = _scalar(actor_grad_norm), _scalar(critic_grad_norm)
    return (out, sc) if scales else out


# what each column is, for the comparisons: equal as numbers, bit-copied, or within a bound
MINMAX = [k for k, n in enumerate(NAMES) if n.endswith("_min") or n.endswith("_max")]
COPIED = [0, 16, 17, 18, 32, 34, 35, 36]
ALPHA = 19
BOUNDED = [k for k in range(N_STATS) if k not in MINMAX and k not in COPIED and k != ALPHA]


def same_number(a, b):
    """Equal as numbers: the same value (so +0 == -0), or both NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def within(a, b, scale, bound):
    """|a - b| <= bound * scale per column, NaN matching NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(a - b) <= bound * np.abs(scale)
    return ok | (np.isnan(a) & np.isnan(b))


def make_inputs(rng, S, A, B, width=None, per=True):
    """Seeded inputs that meet max|x| <= 64 std in every series (normal data): rows [B, width]
    (state | action | reward | filler), q [B, 2], target_q, log_prob [B, 1], weights [B, 1] or None."""
    W = S + A + 1 if width is None else width
    rows = rng.standard_normal((B, W)).astype(np.float32)
    rows[:, :S] = (3.0 * rng.standard_normal((B, S)) + 1.0 + np.arange(S)).astype(np.float32)
    rows[:, S:S + A] = np.tanh(rng.standard_normal((B, A))).astype(np.float32)
    rows[:, S + A] = (0.5 * rng.standard_normal(B) - 0.2).astype(np.float32)
    q = (5.0 * rng.standard_normal((B, 2)) + 2.0).astype(np.float32)
    target_q = (5.0 * rng.standard_normal((B, 1)) + 1.5).astype(np.float32)
    log_prob = (rng.standard_normal((B, 1)) - 1.0).astype(np.float32)
    weights = rng.uniform(0.2, 1.0, (B, 1)).astype(np.float32) if per else None
    return rows, q, target_q, log_prob, weights
