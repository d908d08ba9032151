"""CPU checks of the learning statistics and the agent facade: the reference's recorded values
against the binary64 model (tests/learning_stats_ref.py), the header / library / binding agreement on
pd_sac_learning_stats, its argument checks before any launch (no device needed, the pointers are never
dereferenced), LearningStats on its torch path, and pdenv.agent.SACPyTorch on device="cpu"."""
import csv
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import learning_stats_ref as M
from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's learning_stats key order (sac_pytorch.py:346-397), written out
REFERENCE_KEYS = [
    "step", "state_mean", "state_min", "state_max", "state_std", "state_kurtosis", "action_mean", "action_min",
    "action_max", "action_std", "action_kurtosis", "reward_mean", "reward_min", "reward_max", "reward_std",
    "reward_kurtosis", "critic_loss", "actor_loss", "alpha_loss", "alpha_value", "q_value_mean", "q_value_min",
    "q_value_max", "q_value_std", "log_prob_mean", "log_prob_min", "log_prob_max", "log_prob_std", "target_q_mean",
    "target_q_min", "target_q_max", "target_q_std", "per_beta", "per_mean_weight", "per_max_priority",
    "actor_grad_norm", "critic_grad_norm"]
# the reference's constructor keywords and defaults (sac_pytorch.py:229-270), written out; `device`
# defaults to "cuda" where a device is visible
REFERENCE_KWARGS = dict(
    state_dim=None, action_dim=None, hidden_dim_actor=256, number_of_hidden_layers_actor=2, hidden_dim_critic=256,
    number_of_hidden_layers_critic=2, alpha_initial=0.2, gamma=0.99, tau=0.005, buffer_size=100000, batch_size=256,
    critic_learning_rate=3e-4, actor_learning_rate=3e-4, alpha_learning_rate=3e-4, max_action=1.0, device=None,
    auto_entropy_tuning=True, flight_phase="default", save_stats_frequency=100, use_per=False, per_alpha=0.6,
    per_beta=0.4, per_beta_annealing_steps=100000, per_epsilon=1e-6, use_l1_loss=False, clip_gradients=False,
    max_grad_norm_actor=1.0, max_grad_norm_critic=1.0)
# binary64 two-pass sums of n <= 8232 terms: about 8 n 2^-53 (max|x| / std) relative to the scale,
# under 2^-30 for max|x| <= 64 std (the GPU test's bound; see tests/test_gpu_learning_stats.py)
BOUND = 2.0 ** -30


def _lib():
    import pdenv
    from pdenv import _lib
    return pdenv.load(), _lib


# ------------------------------------------------------------------ the reference against the model
@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_recorded_values_against_the_model(k):
    """The model reproduces what the reference's _track_learning_stats recorded, within 4 times the
    reference's own float32 deviation as the generator measured it (per shape, relative to each
    column's scale); the min and max of a series equal as numbers.  (state_min and state_max are means
    over the dimensions of the per-dimension minima and maxima, which the reference takes in float32,
    np.mean of a float32 array: they are held to the bound like the other means.)"""
    g = golden("ref_learning_stats.npz")
    S, A, B, per = (int(v) for v in g["shapes"][k])
    assert [(2, 1, 261, 1), (5, 4, 17, 1), (8, 2, 512, 0)][k] == (S, A, B, per)
    assert list(g["names"]) == REFERENCE_KEYS == M.NAMES
    keys = list(g[f"keys_{k}"])
    assert keys == REFERENCE_KEYS[:35 if per else 32]          # (the grad norms are logged by update(), not here)
    losses, pr = g[f"losses_{k}"], g[f"per_{k}"]
    model, scale = M.model_row(g[f"rows_{k}"], g[f"q_{k}"], g[f"target_q_{k}"], g[f"log_prob_{k}"], S, A,
                               weights=g[f"weights_{k}"] if per else None, critic_loss=losses[0], actor_loss=losses[1],
                               alpha_loss=losses[2], log_alpha=g[f"log_alpha_{k}"],
                               max_priority=pr[1] if per else None, per_beta=pr[0], step=int(g[f"step_{k}"]), scales=True)
    rec = g[f"recorded_{k}"]
    allowed = 4.0 * float(g[f"max_deviation_{k}"])
    assert 0 < allowed < 1e-5
    for j, name in enumerate(keys):
        c = M.NAMES.index(name)
        if (c in M.MINMAX and not name.startswith("state_")) or c in M.COPIED:
            assert M.same_number(rec[j], model[c]), (name, rec[j], model[c])
        else:
            assert abs(rec[j] - model[c]) <= allowed * abs(scale[c]), (name, rec[j], model[c])


# ------------------------------------------------------------------ header, library and binding
def test_header_library_and_binding_agree():
    L, lib = _lib()
    from pdenv import sac
    txt = open(os.path.join(REPO, "include", "pdenv.h")).read()
    assert re.search(r"^#define PD_SAC_N_STATS 37$", txt, re.M) and lib.SAC_N_STATS == 37 == len(REFERENCE_KEYS)
    assert "sac_pytorch.py:553-634" in txt and "sac_pytorch.py:346-397" in txt
    for name in ("pd_sac_stat_name", "pd_sac_learning_stats"):
        m = re.search(r"^[\w\* ]+\s+\**" + name + r"\(([^;]*)\);", txt, re.M | re.S)
        assert m, f"{name} not declared in include/pdenv.h"
        assert hasattr(L, name) and name in lib.EXPORTS
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), name
    assert L.pd_abi_version() == lib.ABI_VERSION == 11      # additive exports
    names = [L.pd_sac_stat_name(c) for c in range(37)]
    assert [n.decode() for n in names] == REFERENCE_KEYS == list(sac.STAT_NAMES)
    for c in (-1, 37, 38, 2 ** 31 - 1, -2 ** 31):
        assert L.pd_sac_stat_name(c) is None
    assert "pdsacstats" in [os.path.basename(u[1])[:-4] for u in __import__("pdenv.build", fromlist=["x"]).units()]


def _stats(L, **kw):
    ok = C.c_void_p(0x10000)
    a = dict(batch=256, S=2, A=1, rows=ok, width=7, q=ok, target_q=ok, log_prob=ok, weights=ok, critic_loss=ok,
             actor_loss=ok, alpha_loss=ok, log_alpha=ok, max_priority=ok, agn=ok, cgn=ok, per_beta=0.4, step=0, out=ok)
    a.update(kw)
    return L.pd_sac_learning_stats(a["batch"], a["S"], a["A"], a["rows"], a["width"], a["q"], a["target_q"],
                                   a["log_prob"], a["weights"], a["critic_loss"], a["actor_loss"], a["alpha_loss"],
                                   a["log_alpha"], a["max_priority"], a["agn"], a["cgn"], a["per_beta"], a["step"],
                                   a["out"], None)


def test_argument_checks_before_any_launch():
    L, lib = _lib()
    invalid = [dict(batch=0), dict(batch=-3), dict(S=0), dict(S=-1), dict(A=0), dict(A=-1), dict(width=3), dict(width=0),
               dict(width=-7), dict(S=5, A=4, width=9), dict(rows=None), dict(q=None), dict(target_q=None),
               dict(log_prob=None), dict(log_alpha=None), dict(out=None)]
    for kw in invalid:
        assert _stats(L, **kw) == lib.PD_ERR_INVALID, kw
        assert b"pd_sac_learning_stats" in L.pd_last_error()
    unsupported = [dict(S=17, width=40), dict(A=9, width=40), dict(batch=65537), dict(batch=2 ** 40)]
    for kw in unsupported:
        assert _stats(L, **kw) == lib.PD_ERR_UNSUPPORTED, kw
    # a bad argument is INVALID whatever the size
    assert _stats(L, batch=65537, rows=None) == lib.PD_ERR_INVALID
    assert _stats(L, S=17, width=5) == lib.PD_ERR_INVALID


# ------------------------------------------------------------------ LearningStats, torch path, CPU tensors
class _Upd:
    """What LearningStats.record reads of a CriticUpdate / an ActorUpdate."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Buf:
    def __init__(self, beta, max_prio):
        self.beta, self.max_prio_dev = beta, torch.tensor([max_prio], dtype=torch.float32)


def _record(stats, rng, S, A, B, per=True, norms=True, width=None):
    """One record() from seeded inputs; returns the model's row."""
    rows, q, tq, lp, w = M.make_inputs(rng, S, A, B, width=width, per=per)
    sc = rng.standard_normal(5).astype(np.float32)
    la = np.float32(-1.2)
    t = torch.from_numpy
    cu = _Upd(critic_loss=t(sc[0:1]), grad_norm=t(np.abs(sc[3:4])) if norms else None)
    au = _Upd(q=t(q), actor_loss=t(sc[1:2]), alpha_loss=t(sc[2:3]), grad_norm=t(np.abs(sc[4:5])) if norms else None,
              log_alpha=torch.tensor([la]))
    step = stats.step
    stats.record(t(rows), t(tq), cu, au, t(lp), t(w) if per else None, _Buf(0.45, 2.5) if per else None)
    return M.model_row(rows, q, tq, lp, S, A, weights=w, critic_loss=sc[0], actor_loss=sc[1], alpha_loss=sc[2],
                       log_alpha=la, max_priority=2.5 if per else None, actor_grad_norm=abs(sc[4]) if norms else None,
                       critic_grad_norm=abs(sc[3]) if norms else None, per_beta=0.45, step=step, scales=True)


def _check_row(got, model, scale):
    assert M.same_number(got[M.MINMAX], model[M.MINMAX])
    assert M.same_bits(got[M.COPIED], model[M.COPIED])
    ok = M.within(got[M.BOUNDED], model[M.BOUNDED], scale[M.BOUNDED], BOUND)
    assert ok.all(), [(M.NAMES[M.BOUNDED[i]], got[M.BOUNDED[i]], model[M.BOUNDED[i]]) for i in np.nonzero(~ok)[0]]
    assert abs(got[M.ALPHA] - model[M.ALPHA]) <= 2 * np.spacing(np.float32(model[M.ALPHA]))


@pytest.mark.parametrize("S,A,B,per,width", [(2, 1, 261, True, None), (5, 4, 17, True, 16), (8, 2, 512, False, None),
                                            (1, 1, 1, True, None), (16, 8, 2, False, None)])
def test_torch_path_equals_the_model(S, A, B, per, width):
    from pdenv.sac import LearningStats
    stats = LearningStats(S, A, "cpu", capacity=4, kernel=False)
    model, scale = _record(stats, np.random.default_rng(S * 100 + B), S, A, B, per=per, width=width)
    assert stats.last_kernel is False
    _check_row(stats.rows[0], model, scale)
    if B == 1:
        r = stats.columns
        assert r["state_std"][0] == 0 and r["reward_std"][0] == 0 and np.isnan(r["action_kurtosis"][0])


def test_ring_wraps_and_to_dict_omits_absent_keys():
    from pdenv.sac import LearningStats
    rng = np.random.default_rng(5)
    stats = LearningStats(2, 1, "cpu", capacity=3, kernel=False)
    models = [_record(stats, rng, 2, 1, 33, per=False, norms=False) for _ in range(2)]
    stats.flush()                                              # 2 rows out; the next two wrap (slots 2, 0)
    models += [_record(stats, rng, 2, 1, 33, per=False, norms=False) for _ in range(2)]
    assert len(stats) == 4
    d = stats.to_dict()
    assert list(d) == REFERENCE_KEYS[:32]                      # no PER keys, no grad-norm keys
    assert d["step"] == [0, 1, 2, 3] and all(isinstance(v, int) for v in d["step"])
    for r, (model, scale) in zip(stats.rows, models):
        _check_row(r, model, scale)
    models += [_record(stats, rng, 2, 1, 33, per=True, norms=True) for _ in range(4)]   # fills the ring: flushes itself
    assert stats._flushed == 7                                 # (4 by to_dict, then 3 more filled the ring)
    assert list(stats.to_dict()) == REFERENCE_KEYS
    assert list(stats.columns) == REFERENCE_KEYS and stats.rows.shape == (8, 37)
    for r, (model, scale) in zip(stats.rows, models):
        _check_row(r, model, scale)
    assert np.isnan(stats.columns["per_beta"][:4]).all() and (stats.columns["per_beta"][4:] == 0.45).all()


def test_save_csv_writes_one_header_then_appends(tmp_path):
    from pdenv.sac import LearningStats
    rng = np.random.default_rng(6)
    stats = LearningStats(2, 1, "cpu", capacity=8, kernel=False)
    path = str(tmp_path / "sub" / "stats.csv")
    assert stats.save_csv(path) == 0 and not os.path.exists(path)
    for _ in range(3):
        _record(stats, rng, 2, 1, 20)
    assert stats.save_csv(path) == 3
    for _ in range(2):
        _record(stats, rng, 2, 1, 20)
    assert stats.save_csv(path) == 2 and stats.save_csv(path) == 0
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == REFERENCE_KEYS and len(lines) == 6
    assert [int(float(r[0])) for r in lines[1:]] == [0, 1, 2, 3, 4]
    got = np.array([[float(v) for v in r] for r in lines[1:]])
    assert np.allclose(got, stats.rows, rtol=1e-12, atol=0, equal_nan=True)


# ------------------------------------------------------------------ the agent on the CPU
def _agent(**kw):
    from pdenv.agent import SACPyTorch
    a = dict(hidden_dim_actor=128, hidden_dim_critic=128, batch_size=16, buffer_size=256, device="cpu",
             save_stats_frequency=1000)
    a.update(kw)
    return SACPyTorch(2, 1, **a)


def _fill(agent, n, seed=0):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        s = rng.standard_normal(agent.state_dim)
        a = agent.select_action(s)
        assert isinstance(a, np.ndarray) and a.shape == (agent.action_dim,)
        agent.replay_buffer.add(s, a, float(rng.standard_normal()), rng.standard_normal(agent.state_dim), False)


def test_agent_constructor_keywords_are_the_references():
    from pdenv.agent import SACPyTorch
    import pdenv
    assert pdenv.SACPyTorch is SACPyTorch
    ps = inspect.signature(SACPyTorch.__init__).parameters
    assert list(ps)[1:] == list(REFERENCE_KWARGS)
    for name, default in REFERENCE_KWARGS.items():
        if name in ("state_dim", "action_dim"):
            assert ps[name].default is inspect.Parameter.empty
        elif name == "device":
            assert ps[name].default == ("cuda" if torch.cuda.is_available() else "cpu")
        else:
            assert ps[name].default == default and type(ps[name].default) is type(default), name


def test_agent_update_and_learning_stats(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    agent = _agent(use_per=True, clip_gradients=True)
    assert os.listdir(tmp_path) == []                          # no directory at construction
    assert agent.log_alpha.dtype == torch.float32 and agent.log_alpha.shape == (1,) and agent.target_entropy == -1
    assert abs(agent.alpha.detach().item() - 0.2) < 1e-7
    _fill(agent, 15)
    before = [p.clone() for p in agent.actor.parameters()]
    agent.update()                                             # below batch_size: nothing happens
    assert agent.updates == 0 and agent.learning_stats["step"] == []
    assert all(torch.equal(a, b) for a, b in zip(before, agent.actor.parameters()))
    _fill(agent, 25, seed=1)
    for _ in range(5):
        agent.update()
    d = agent.learning_stats
    assert agent.updates == 5 and d["step"] == [0, 1, 2, 3, 4]
    assert list(d) == REFERENCE_KEYS and all(len(v) == 5 for v in d.values())
    assert np.isfinite(np.array([d[k] for k in REFERENCE_KEYS if not k.endswith("kurtosis")])).all()
    assert not any(torch.equal(a, b) for a, b in zip(before, agent.actor.parameters()))
    assert d["alpha_value"][-1] == pytest.approx(agent.alpha.detach().item(), rel=1e-6)
    assert d["per_max_priority"][-1] == agent.replay_buffer.max_priority
    # without PER and clipping the dict has the reference's 32 keys
    plain = _agent()
    _fill(plain, 20)
    plain.update()
    assert list(plain.learning_stats) == REFERENCE_KEYS[:32] and plain.learning_stats["step"] == [0]
    # save_learning_stats: the reference's path rules
    agent.save_learning_stats(run_id="r7")
    assert os.path.isfile("data/agent_saves/PyTorchSAC/default/learning_stats/sac_learning_stats_r7.csv")
    agent.run_dir = str(tmp_path / "run")
    agent.update()
    agent.save_learning_stats()
    with open(tmp_path / "run" / "learning_stats" / "sac_learning_stats.csv") as f:
        assert len(f.read().splitlines()) == 2                 # the header and the one row not yet saved


def test_agent_saves_every_save_stats_frequency_updates(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    agent = _agent(save_stats_frequency=2)
    agent.run_id = "abc"
    _fill(agent, 20)
    for _ in range(5):
        agent.update()
    with open("data/agent_saves/PyTorchSAC/default/learning_stats/sac_learning_stats_abc.csv") as f:
        lines = f.read().splitlines()
    assert len(lines) == 5 and lines[0].split(",") == REFERENCE_KEYS[:32]


def test_agent_save_then_load(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    agent = _agent(use_per=True)
    _fill(agent, 30)
    for _ in range(3):
        agent.update()
    path = str(tmp_path / "ck" / "agent")
    agent.save(path)
    assert os.path.isfile(path) and os.path.isfile(path + "_learning_stats.csv")
    ck = torch.load(path)
    assert list(ck) == ["actor", "critic", "critic_target", "log_alpha", "actor_optimizer", "critic_optimizer",
                        "alpha_optimizer", "updates"]
    torch.manual_seed(2)
    other = _agent(use_per=True)
    la = other.log_alpha
    other.load(path)
    assert other.updates == 3 and other.stats.step == 3
    assert other.log_alpha is la and torch.equal(la, agent.log_alpha) and la.dtype == torch.float32
    for name in ("actor", "critic", "critic_target"):
        for (k, a), (_, b) in zip(getattr(agent, name).state_dict().items(), getattr(other, name).state_dict().items()):
            assert torch.equal(a, b), (name, k)
    for name in ("actor_optimizer", "critic_optimizer", "alpha_optimizer"):
        sa, sb = getattr(agent, name).state_dict(), getattr(other, name).state_dict()
        assert sa["param_groups"] == sb["param_groups"] and list(sa["state"]) == list(sb["state"])
        for k in sa["state"]:
            for f in sa["state"][k]:
                assert torch.equal(torch.as_tensor(sa["state"][k][f]), torch.as_tensor(sb["state"][k][f])), (name, k, f)


def test_agent_loads_a_reference_checkpoint_log_alpha(tmp_path, monkeypatch):
    """The reference saves log_alpha as a 0-dim float64 tensor: load() copies the value into the
    agent's own float32 tensor, which stays the optimizer's parameter and the kernels' pointer."""
    monkeypatch.chdir(tmp_path)
    agent = _agent()
    path = str(tmp_path / "agent")
    agent.save(path)
    ck = torch.load(path)
    ck["log_alpha"] = torch.tensor(-0.7312345678, dtype=torch.float64, requires_grad=True)
    torch.save(ck, path)
    la, ptr = agent.log_alpha, agent.log_alpha.data_ptr()
    agent.load(path)
    assert agent.log_alpha is la and la.data_ptr() == ptr and la.dtype == torch.float32 and la.shape == (1,)
    assert la.requires_grad and la.item() == np.float32(-0.7312345678)
    assert agent.alpha_optimizer.param_groups[0]["params"][0] is la
    assert agent.td_target.log_alpha is la and agent.actor_update.log_alpha is la
