"""The reference's SAC agent, SACPyTorch (sac_pytorch.py:227-724), on the fused update.

The driver constructs `SACPyTorch(state_dim, action_dim, ...)` and uses .select_action, .update(),
.replay_buffer.add, .save / .load, .learning_stats and .save_learning_stats; this class has the same
constructor keywords with the same defaults and the same members.  update() is pdenv.sac.sac_update
-- the prioritized sample, the TD target, the critic, actor and temperature steps and the priority
update as a fixed sequence of launches -- plus one pd_sac_learning_stats launch for the update's
learning_stats row; between two saves of the statistics nothing is read back from the device.
"""
import os
from datetime import datetime

import numpy as np
import torch

from . import _lib as L
from .sac import (Actor, ActorUpdate, Critic, CriticUpdate, DevicePrioritizedReplayBuffer, DeviceReplayBuffer,
                  KernelPrioritizedReplayBuffer, LearningStats, SACCollector, TdTarget, evaluate_agent, sac_update)


class SACPyTorch:
    """sac_pytorch.py:227-724.  Differences a caller can see:

    * log_alpha is a one-element float32 tensor on the device (the reference's is 0-dim float64): the
      kernels read it in place.  load() takes either and copies the value into the existing tensor.
    * replay_buffer is a device buffer: KernelPrioritizedReplayBuffer under use_per on a HIP device,
      DevicePrioritizedReplayBuffer under use_per on the CPU, DeviceReplayBuffer otherwise; add()
      takes the reference's arguments.
    * learning_stats is a property: the dict of lists, read from the device ring (a flush).
    * no directory is created at construction, only when something is saved.
    * the sampling streams are the kernels' Philox draws, not NumPy's and torch's global generators;
      reseed(seed) sets them.
    On device="cpu" every step takes the torch fallbacks of pdenv.sac: usable without a GPU, slowly."""

    def __init__(
        self,
        state_dim: int,
        action_dim: int,
        hidden_dim_actor: int = 256,
        number_of_hidden_layers_actor: int = 2,
        hidden_dim_critic: int = 256,
        number_of_hidden_layers_critic: int = 2,
        alpha_initial: float = 0.2,
        gamma: float = 0.99,
        tau: float = 0.005,
        buffer_size: int = 100000,
        batch_size: int = 256,
        critic_learning_rate: float = 3e-4,
        actor_learning_rate: float = 3e-4,
        alpha_learning_rate: float = 3e-4,
        max_action: float = 1.0,
        device: str = "cuda" if torch.cuda.is_available() else "cpu",
        auto_entropy_tuning: bool = True,
        flight_phase: str = "default",
        save_stats_frequency: int = 100,
        use_per: bool = False,
        per_alpha: float = 0.6,
        per_beta: float = 0.4,
        per_beta_annealing_steps: int = 100000,
        per_epsilon: float = 1e-6,
        use_l1_loss: bool = False,
        clip_gradients: bool = False,
        max_grad_norm_actor: float = 1.0,
        max_grad_norm_critic: float = 1.0
    ):
        self.state_dim = state_dim
        self.action_dim = action_dim
        self.gamma = gamma
        self.tau = tau
        self.batch_size = batch_size
        self.max_action = max_action
        self.device = device
        self.auto_entropy_tuning = auto_entropy_tuning
        self.flight_phase = flight_phase
        self.save_stats_frequency = save_stats_frequency
        self.use_per = use_per
        self.use_l1_loss = use_l1_loss
        self.clip_gradients = clip_gradients
        self.max_grad_norm_actor = max_grad_norm_actor
        self.max_grad_norm_critic = max_grad_norm_critic
        dev = torch.device(device)

        self.actor = Actor(state_dim, action_dim, hidden_dim_actor, number_of_hidden_layers_actor, max_action).to(dev)
        self.critic = Critic(state_dim, action_dim, hidden_dim_critic, number_of_hidden_layers_critic).to(dev)
        self.critic_target = Critic(state_dim, action_dim, hidden_dim_critic, number_of_hidden_layers_critic).to(dev)
        self.critic_target.load_state_dict(self.critic.state_dict())

        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=actor_learning_rate)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=critic_learning_rate)
        self.log_alpha = torch.tensor([np.log(alpha_initial)], dtype=torch.float32, device=dev, requires_grad=True)
        self.alpha_optimizer = torch.optim.Adam([self.log_alpha], lr=alpha_learning_rate)
        self.target_entropy = -action_dim

        if use_per:
            per = dict(alpha=per_alpha, beta=per_beta, beta_annealing_steps=per_beta_annealing_steps, epsilon=per_epsilon)
            if dev.type == "cuda" and batch_size <= L.PER_MAX_BATCH:
                self.replay_buffer = KernelPrioritizedReplayBuffer(buffer_size, state_dim, action_dim, dev, **per)
            else:
                self.replay_buffer = DevicePrioritizedReplayBuffer(buffer_size, state_dim, action_dim, dev, **per)
        else:
            self.replay_buffer = DeviceReplayBuffer(buffer_size, state_dim, action_dim, dev)

        self.td_target = TdTarget(self.actor, self.critic_target, self.log_alpha, gamma)
        self.critic_update = CriticUpdate(self.critic, self.critic_target, self.critic_optimizer, tau=tau,
                                          use_l1_loss=use_l1_loss,
                                          max_grad_norm=max_grad_norm_critic if clip_gradients else None)
        self.actor_update = ActorUpdate(self.actor, self.critic, self.log_alpha, self.actor_optimizer,
                                        self.alpha_optimizer if auto_entropy_tuning else None,
                                        target_entropy=self.target_entropy,
                                        max_grad_norm=max_grad_norm_actor if clip_gradients else None)
        self.stats = LearningStats(state_dim, action_dim, dev, capacity=save_stats_frequency)
        self.updates = 0

    def reseed(self, seed):
        """The seed of the sampling kernels' Philox streams (the prioritized sample, the TD target's
        and the actor step's rsample noise); 0 at construction."""
        self.td_target.seed = self.actor_update.seed = int(seed)
        if hasattr(self.replay_buffer, "seed"):
            self.replay_buffer.seed = int(seed)

    @property
    def alpha(self):
        return self.log_alpha.exp()

    def select_action(self, state, deterministic=False):
        with torch.no_grad():
            state = torch.as_tensor(np.asarray(state), dtype=torch.float32).reshape(1, -1).to(self.device)
            action, _ = self.actor.sample(state, deterministic, with_log_prob=False)
            return action.cpu().numpy().flatten()

    def update(self):
        if len(self.replay_buffer) < self.batch_size:
            return
        sac_update(self.replay_buffer, self.td_target, self.critic_update, self.actor_update, self.batch_size,
                   stats=self.stats)
        self.updates += 1
        if self.updates % self.save_stats_frequency == 0:
            self.save_learning_stats(run_id=getattr(self, "run_id", None))

    @property
    def learning_stats(self):
        """{key: list}, the reference's dict (the PER keys under use_per, the grad-norm keys under
        clip_gradients); reading it brings the rows still on the device over."""
        d = self.stats.to_dict()
        for name, wanted in (("per_beta", self.use_per), ("per_mean_weight", self.use_per),
                             ("per_max_priority", self.use_per), ("actor_grad_norm", self.clip_gradients),
                             ("critic_grad_norm", self.clip_gradients)):
            if wanted:
                d.setdefault(name, [])
            else:
                d.pop(name, None)
        return d

    def _default_path(self, kind, stem, run_id):
        if run_id is None:
            run_id = datetime.now().strftime("%Y%m%d_%H%M%S")
        return f"data/agent_saves/PyTorchSAC/{self.flight_phase}/{kind}/{stem}_{run_id}"

    def save_learning_stats(self, filename=None, run_id=None):
        run_dir = getattr(self, "run_dir", None)
        if filename is None:
            if run_dir:
                filename = f"{run_dir}/learning_stats/sac_learning_stats.csv"
            else:
                filename = self._default_path("learning_stats", "sac_learning_stats", run_id) + ".csv"
        if len(self.stats) == 0:
            print("No data")
            return
        self.stats.save_csv(filename)

    def save(self, filename=None, run_id=None):
        run_dir = getattr(self, "run_dir", None)
        if filename is None:
            if run_dir:
                filename = f"{run_dir}/agent_saves/sac_pytorch"
            else:
                filename = self._default_path("saves", "sac_pytorch", run_id)
        d = os.path.dirname(filename)
        if d:
            os.makedirs(d, exist_ok=True)
        self.save_learning_stats(f"{filename}_learning_stats.csv", run_id)
        torch.save({
            "actor": self.actor.state_dict(),
            "critic": self.critic.state_dict(),
            "critic_target": self.critic_target.state_dict(),
            "log_alpha": self.log_alpha,
            "actor_optimizer": self.actor_optimizer.state_dict(),
            "critic_optimizer": self.critic_optimizer.state_dict(),
            "alpha_optimizer": self.alpha_optimizer.state_dict(),
            "updates": self.updates
        }, filename)
        print(f"Model saved to {filename}")

    def load(self, filename):
        checkpoint = torch.load(filename, map_location=self.device)
        self.actor.load_state_dict(checkpoint["actor"])
        self.critic.load_state_dict(checkpoint["critic"])
        self.critic_target.load_state_dict(checkpoint["critic_target"])
        # in place: the kernels' pointer and the optimizer's parameter stay valid (the reference's
        # log_alpha is 0-dim float64; copy_ casts)
        with torch.no_grad():
            self.log_alpha.copy_(torch.as_tensor(checkpoint["log_alpha"]).detach().reshape(self.log_alpha.shape))
        self.actor_optimizer.load_state_dict(checkpoint["actor_optimizer"])
        self.critic_optimizer.load_state_dict(checkpoint["critic_optimizer"])
        self.alpha_optimizer.load_state_dict(checkpoint["alpha_optimizer"])
        self.updates = checkpoint["updates"]
        self.stats.step = int(self.updates)
        print(f"Model loaded from {filename}")

    def collector(self, env, **kw):
        """A SACCollector of this agent's actor into its replay buffer (the vectorised loop:
        agent.collector(env).collect(K), then agent.update())."""
        return SACCollector(env, self.actor, self.replay_buffer, **kw)

    def evaluate(self, env, **kw):
        """pdenv.sac.evaluate_agent with this agent's actor."""
        return evaluate_agent(self.actor, env, **kw)
