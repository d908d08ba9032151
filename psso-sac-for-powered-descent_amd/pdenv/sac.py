"""SAC data path on the device (SURVEY config c5): the reference's actor drives N envs per GPU,
transitions are all-gathered over RCCL into a device replay buffer on the learner rank.

The reference steps ONE env per process and adds one transition per step to a numpy buffer
(sac_pytorch_powered_descent.py:160-183, sac_pytorch.py:12-49).  Here every rank steps its own
env shard through libpdenv, builds the transition slab [n_local, s|a|r|s'|done] (28 B per env
for the pure-throttle task), and `all_gather_into_tensor` (backend "nccl" = RCCL over xGMI)
concatenates the slabs in rank order; the learner rank appends them to its ring buffer.  The
learner itself (critic/actor updates) is the caller's, as in the reference.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from .env import _ptr, _stream


class Actor(nn.Module):
    """sac_pytorch.py:129-179: shared MLP (ReLU), mean and log_std heads, tanh squashing."""

    def __init__(self, state_dim, action_dim, hidden_dim=256, n_hidden_layers=2, max_action=1.0,
                 log_std_min=-20.0, log_std_max=2.0):
        super().__init__()
        self.max_action, self.log_std_min, self.log_std_max = max_action, log_std_min, log_std_max
        layers = [nn.Linear(state_dim, hidden_dim), nn.ReLU()]
        for _ in range(n_hidden_layers - 1):
            layers += [nn.Linear(hidden_dim, hidden_dim), nn.ReLU()]
        self.shared_net = nn.Sequential(*layers)
        self.mean = nn.Linear(hidden_dim, action_dim)
        self.log_std = nn.Linear(hidden_dim, action_dim)

    def forward(self, state):
        f = self.shared_net(state)
        return self.mean(f), torch.clamp(self.log_std(f), self.log_std_min, self.log_std_max)

    def sample(self, state, deterministic=False, generator=None, with_log_prob=True):
        """with_log_prob=False skips the log-probability (select_action discards it,
        sac_pytorch_powered_descent.py / sac_pytorch.py:404-409): same action, fewer kernels."""
        mean, log_std = self(state)
        if deterministic:
            return torch.tanh(mean) * self.max_action, None
        std = log_std.exp()
        eps = torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
        x = mean + std * eps                                   # Normal(mean, std).rsample()
        action = torch.tanh(x)
        if not with_log_prob:
            return action * self.max_action, None
        log_prob = (-((x - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727
                    - torch.log(1 - action.pow(2) + 1e-6)).sum(-1, keepdim=True)
        return action * self.max_action, log_prob


class DeviceReplayBuffer:
    """The reference's uniform ReplayBuffer (sac_pytorch.py:12-49) as device tensors.
    add_batch appends B transitions at once (ring, oldest overwritten)."""

    def __init__(self, capacity, state_dim, action_dim, device):
        self.capacity, self.state_dim, self.action_dim = int(capacity), state_dim, action_dim
        self.width = 2 * state_dim + action_dim + 2
        self.data = torch.zeros(self.capacity, self.width, dtype=torch.float32, device=device)
        self.position = 0
        self.size = 0
        self.last_rows = None       # the [B, W] rows of the last sample
        # the ring's position and size on the device (int64: position, size, pd_step_sac_ring's
        # workgroup counter): the collection kernel writes its rows there and advances them, the
        # host mirrors (position, size) by note_appended
        self.state_dev = torch.zeros(3, dtype=torch.int64, device=device)

    def _sync_state_dev(self):
        # device-side fills (no host tensor, so no blocking pageable copy on the step's stream)
        self.state_dev[0].fill_(self.position)
        self.state_dev[1].fill_(self.size)
        self.state_dev[2].zero_()

    def note_appended(self, b):
        """The host mirror of b rows appended on the device (pd_step_sac_ring)."""
        self.position = (self.position + b) % self.capacity
        self.size = min(self.size + b, self.capacity)

    def rows(self, start, b):
        """The b ring rows from start (a view unless they wrap)."""
        end = start + b
        if end <= self.capacity:
            return self.data[start:end]
        return torch.cat([self.data[start:], self.data[:end - self.capacity]])

    def add_batch(self, slab):
        """slab [B, 2S + A + 2] = state | action | reward | next_state | done (float32)."""
        b = slab.shape[0]
        if b > self.capacity:
            slab, b = slab[-self.capacity:], self.capacity
        end = self.position + b
        if end <= self.capacity:
            self.data[self.position:end] = slab
        else:
            k = self.capacity - self.position
            self.data[self.position:] = slab[:k]
            self.data[:b - k] = slab[k:]
        self.position = end % self.capacity
        self.size = min(self.size + b, self.capacity)
        self._sync_state_dev()

    def add(self, state, action, reward, next_state, done):
        """The reference's one-transition add (sac_pytorch.py:27-35)."""
        row = torch.cat([torch.as_tensor(state, dtype=torch.float32).reshape(-1),
                         torch.as_tensor(action, dtype=torch.float32).reshape(-1),
                         torch.tensor([float(reward)]),
                         torch.as_tensor(next_state, dtype=torch.float32).reshape(-1),
                         torch.tensor([float(done)])]).to(self.data.device)
        self.add_batch(row[None])

    def sample(self, batch_size, generator=None):
        """Uniform indices in [0, size) (np.random.randint, sac_pytorch.py:37-46)."""
        idx = torch.randint(0, self.size, (batch_size,), device=self.data.device, generator=generator)
        d = self.data[idx]
        self.last_rows = d          # the [B, W] tensor behind the views (TdTarget's input)
        S, A = self.state_dim, self.action_dim
        return (d[:, :S], d[:, S:S + A], d[:, S + A:S + A + 1], d[:, S + A + 1:2 * S + A + 1],
                d[:, 2 * S + A + 1:])

    def __len__(self):
        return self.size


class DevicePrioritizedReplayBuffer(DeviceReplayBuffer):
    """The reference's PrioritizedReplayBuffer (sac_pytorch.py:51-127; the SAC driver's buffer,
    use_per=True) as device tensors.

    New transitions get the current max priority.  sample() draws batch_size distinct indices
    with probability proportional to priority**alpha without replacement -- the distribution of
    np.random.choice(size, batch, replace=False, p=probs) -- by the Gumbel-top-k construction
    (top-k of alpha*log(priority) + Gumbel noise), returns importance weights
    (size*probs)**(-beta) / max, and anneals beta."""

    def __init__(self, capacity, state_dim, action_dim, device, alpha=0.6, beta=0.4,
                 beta_annealing_steps=100000, epsilon=1e-6):
        super().__init__(capacity, state_dim, action_dim, device)
        self.alpha, self.beta, self.epsilon = alpha, beta, epsilon
        self.beta_increment = (1.0 - beta) / beta_annealing_steps
        self.priorities = torch.zeros(self.capacity, dtype=torch.float32, device=device)
        self.max_priority = 1.0
        self.max_prio_dev = torch.ones(1, dtype=torch.float32, device=device)   # (read by pd_step_sac_ring)

    def add_batch(self, slab):
        b = min(slab.shape[0], self.capacity)
        if self.position + b <= self.capacity:                 # no wrap: one fill
            self.priorities[self.position:self.position + b] = self.max_priority
        else:                                                  # wrap: the tail, then the head
            k = self.capacity - self.position
            self.priorities[self.position:] = self.max_priority
            self.priorities[:b - k] = self.max_priority
        super().add_batch(slab)

    def sample(self, batch_size, generator=None):
        if self.size == 0:
            return None
        pr = self.priorities[:self.size].double()
        probs = pr ** self.alpha
        probs = probs / probs.sum()
        u = torch.rand(self.size, dtype=torch.float64, device=self.data.device, generator=generator)
        gumbel = -torch.log(-torch.log(u.clamp_min(1e-300)))
        idx = torch.topk(torch.log(probs) + gumbel, batch_size).indices
        w = (self.size * probs[idx]) ** (-self.beta)
        w = (w / w.max()).float().reshape(-1, 1)
        self.beta = min(1.0, self.beta + self.beta_increment)
        d = self.data[idx]
        self.last_rows = d
        S, A = self.state_dim, self.action_dim
        return (d[:, :S], d[:, S:S + A], d[:, S + A:S + A + 1], d[:, S + A + 1:2 * S + A + 1],
                d[:, 2 * S + A + 1:], w, idx)

    def update_priorities(self, indices, td_errors):
        """sac_pytorch.py:120-124: priority = |td| + epsilon; max_priority tracks the largest."""
        p = td_errors.detach().reshape(-1).abs().float() + self.epsilon
        self.priorities[indices] = p
        self.max_priority = max(self.max_priority, float(p.max()))
        self.max_prio_dev.fill_(self.max_priority)


class KernelPrioritizedReplayBuffer(DevicePrioritizedReplayBuffer):
    """DevicePrioritizedReplayBuffer with the learner's round trip on the library's kernels: sample
    is one pd_per_sample call (its own Philox draws keyed by (seed, draw); indices, importance
    weights and the gathered rows), update_priorities one pd_per_update call that raises the
    device-side maximum -- neither reads anything back, so a learner update makes no host
    synchronisation.  max_priority lives on the device (max_prio_dev, which the collection kernels
    read): reading the property is the one place that synchronises, setting it fills the device
    value, and add_batch fills the new rows' priorities from the device value.  SACCollector takes
    the class as it takes its parent.

    sample(batch_size) returns the parent's 7-tuple; the first five are views of one [B, W] tensor.
    That tensor, the weights, the indices (and the keys) are owned by the buffer and reused: the next
    sample of the same batch size overwrites them, as the collector's slab is overwritten by its next
    step -- clone what must outlive it."""

    def __init__(self, capacity, state_dim, action_dim, device, alpha=0.6, beta=0.4,
                 beta_annealing_steps=100000, epsilon=1e-6, seed=0):
        super().__init__(capacity, state_dim, action_dim, device, alpha=alpha, beta=beta,
                         beta_annealing_steps=beta_annealing_steps, epsilon=epsilon)
        self.lib = L.load()
        self.seed = int(seed)
        self.draws = 0                # the default `draw` of the next sample
        self._out = {}                # batch size -> (indices, weights, rows, info, scratch)
        self._keys = None

    @property
    def max_priority(self):
        return float(self.max_prio_dev.item())

    @max_priority.setter
    def max_priority(self, value):
        dev = self.__dict__.get("max_prio_dev")   # (the parent's constructor assigns before it exists)
        if dev is not None:
            dev.fill_(float(value))

    def add_batch(self, slab):
        b = min(slab.shape[0], self.capacity)
        if self.position + b <= self.capacity:
            self.priorities[self.position:self.position + b] = self.max_prio_dev
        else:
            k = self.capacity - self.position
            self.priorities[self.position:] = self.max_prio_dev
            self.priorities[:b - k] = self.max_prio_dev
        DeviceReplayBuffer.add_batch(self, slab)

    def _buffers(self, b):
        out = self._out.get(b)
        if out is None:
            dev = self.data.device
            nbytes = int(self.lib.pd_per_sample_scratch_bytes(self.capacity, b))
            out = (torch.empty(b, dtype=torch.int64, device=dev), torch.empty(b, dtype=torch.float32, device=dev),
                   torch.empty(b, self.width, dtype=torch.float32, device=dev),
                   torch.empty(4, dtype=torch.int32, device=dev),
                   torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev))
            self._out[b] = out
        return out

    def sample(self, batch_size, draw=None, check=False, keys=False):
        """batch_size distinct rows, priority**alpha-proportional without replacement; beta is annealed
        as in the parent.  draw: the Philox draw number (default: a counter that advances by one per
        call); the sample depends on (seed, draw, priorities) only.  check=True reads the kernel's
        info words back (a synchronisation): ValueError when fewer than batch_size rows have a
        positive priority (numpy's error; without check such a sample ends in index -1, weight 0 and
        zero rows), RuntimeError on an internal overflow.  keys=True appends the [size] float64 key
        tensor to the result.  The returned tensors are overwritten by the next sample."""
        if self.size == 0:
            return None
        b = int(batch_size)
        if b > self.size:
            raise ValueError(f"cannot take a larger sample ({b}) than the buffer holds ({self.size}) without replacement")
        idx, w, rows, info, scratch = self._buffers(b)
        if keys and self._keys is None:
            self._keys = torch.empty(self.capacity, dtype=torch.float64, device=self.data.device)
        if draw is None:
            draw = self.draws
            self.draws += 1
        L.check(self.lib.pd_per_sample(_ptr(self.priorities), self.size, b, float(self.alpha), float(self.beta),
                                       self.seed & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), _ptr(self.data),
                                       self.width, _ptr(idx), _ptr(w), _ptr(rows), _ptr(self._keys) if keys else None,
                                       _ptr(info), _ptr(scratch), scratch.numel() * 8, _stream(self.data.device)))
        self.beta = min(1.0, self.beta + self.beta_increment)
        if check:
            filled, finite, overflow, _ = info.tolist()
            if overflow:
                raise RuntimeError("pd_per_sample: the candidate list overflowed")
            if filled < b:
                raise ValueError(f"fewer rows with a positive priority ({finite}) than the sample size ({b})")
        self.last_rows = rows
        S, A = self.state_dim, self.action_dim
        out = (rows[:, :S], rows[:, S:S + A], rows[:, S + A:S + A + 1], rows[:, S + A + 1:2 * S + A + 1],
               rows[:, 2 * S + A + 1:], w.reshape(-1, 1), idx)
        return out + (self._keys[:self.size],) if keys else out

    def update_priorities(self, indices, td_errors):
        """sac_pytorch.py:120-124 on the device: priority = |td| + epsilon at the (distinct) indices,
        the device-side maximum raised; indices outside [0, size) -- the -1 of a short sample -- are
        skipped."""
        td = td_errors.detach().reshape(-1).float().contiguous()   # (the kernel takes the absolute value)
        idx = indices.reshape(-1).to(torch.int64).contiguous()
        if td.numel() != idx.numel():
            raise ValueError("update_priorities: as many td errors as indices are required")
        L.check(self.lib.pd_per_update(_ptr(self.priorities), self.size, _ptr(idx), _ptr(td), int(idx.numel()),
                                       float(self.epsilon), _ptr(self.max_prio_dev), _stream(self.data.device)))


def transition_slab(obs, action, reward, next_obs, done):
    """[N, 2S + A + 2] float32: state | action | reward | next_state | done (done, not truncated,
    as the driver stores it: sac_pytorch_powered_descent.py:170-176)."""
    return torch.cat([obs.float(), action.float(), reward.float()[:, None], next_obs.float(),
                      done.float()[:, None]], dim=1).contiguous()


def gather_slabs(slab, dist=None):
    """All ranks' slabs concatenated in rank order (all_gather_into_tensor; RCCL on GPU ranks)."""
    if dist is None or not dist.is_initialized():
        return slab
    out = torch.empty((dist.get_world_size() * slab.shape[0], slab.shape[1]), dtype=slab.dtype,
                      device=slab.device)
    dist.all_gather_into_tensor(out, slab)
    return out


def step_major(gathered):
    """The ranks' collection slabs [world, k, N, W], as all_gather_into_tensor stacks them, as rows
    [k * world * N, W] in step-major order: step 0 of every rank in rank order, then step 1, ... --
    the order k per-step gathers (gather_slabs) append in."""
    world, k, n, w = gathered.shape
    return gathered.permute(1, 0, 2, 3).reshape(k * world * n, w)


class ActorKernel:
    """The Actor's forward pass as one pd_sac_actor launch (the shared MLP on MFMA and both heads,
    activations in LDS): obs [N, S] float32 -> heads [N, 2A] (mean | log_std, unclamped).  Reads
    the actor's parameter tensors in place (no copies: an optimizer step or an in-place update of
    any kind is seen by the next call; a captured graph keeps the parameter addresses it saw, so
    replacing a parameter tensor -- `.data = ...` -- needs a re-capture).  supported(actor) tells
    whether the shapes fit the kernel (hidden 128/256/512, <= 8 hidden layers, S <= 16, A <= 8,
    float32 parameters on the device)."""

    def __init__(self, actor):
        self.actor = actor
        self.lib = L.load()
        lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)]
        self.S, self.H, self.A = lins[0].in_features, lins[0].out_features, actor.mean.out_features
        self.nl = len(lins)
        self.params = [t for m in lins for t in (m.weight, m.bias)] + [actor.mean.weight, actor.mean.bias,
                                                                       actor.log_std.weight, actor.log_std.bias]
        self._ptrs = (C.c_void_p * len(self.params))()

    @staticmethod
    def supported(actor):
        lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)]
        acts = [m for m in actor.shared_net if not isinstance(m, nn.Linear)]
        if not lins or len(lins) > 8 or any(not isinstance(m, nn.ReLU) for m in acts) or len(acts) != len(lins):
            return False
        H = lins[0].out_features
        ps = [p for m in lins for p in (m.weight, m.bias)] + list(actor.mean.parameters()) + list(actor.log_std.parameters())
        return (H in (128, 256, 512) and lins[0].in_features <= 16 and actor.mean.out_features <= 8
                and all(m.in_features == H and m.out_features == H for m in lins[1:])
                and all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and p.data_ptr() % 16 == 0
                        for p in ps))

    def ptrs(self):
        """The parameter pointers as pd_sac_actor / pd_step_sac_fused take them (read now: an
        in-place update keeps them, a replaced tensor is picked up here)."""
        for k, t in enumerate(self.params):
            self._ptrs[k] = t.data_ptr()
        return self._ptrs

    def __call__(self, obs, heads):
        L.check(self.lib.pd_sac_actor(int(obs.shape[0]), self.S, self.H, self.nl, self.A, _ptr(obs), self.ptrs(),
                                      _ptr(heads), _stream(obs.device)))
        return heads


class Critic(nn.Module):
    """sac_pytorch.py:181-221: twin Q nets on cat([state, action]), each Linear(S + A, H) ReLU,
    (Linear(H, H) ReLU) x (n_hidden_layers - 1), Linear(H, 1).  The members are named q1 / q2, so a
    reference checkpoint's critic / critic_target state dict loads (keys q1.0.weight ...)."""

    def __init__(self, state_dim, action_dim, hidden_dim=256, n_hidden_layers=2):
        super().__init__()

        def net():
            layers = [nn.Linear(state_dim + action_dim, hidden_dim), nn.ReLU()]
            for _ in range(n_hidden_layers - 1):
                layers += [nn.Linear(hidden_dim, hidden_dim), nn.ReLU()]
            return nn.Sequential(*layers, nn.Linear(hidden_dim, 1))

        self.state_dim, self.action_dim = state_dim, action_dim
        self.q1, self.q2 = net(), net()

    def forward(self, state, action):
        sa = torch.cat([state, action], dim=1)
        return self.q1(sa), self.q2(sa)


def _q_linears(net):
    """(hidden Linear layers, output Linear, whether the stack is Linear-ReLU ... Linear(H, 1))."""
    mods = list(net)
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    ok = (len(mods) == 2 * len(lins) - 1 and len(lins) >= 2
          and all(isinstance(m, nn.Linear if k % 2 == 0 else nn.ReLU) for k, m in enumerate(mods)))
    return lins[:-1], (lins[-1] if lins else None), ok


class CriticKernel:
    """The Critic's forward pass as one pd_sac_critic launch (Q1 and Q2 in workgroups of their own,
    ActorKernel's MLP code): states [N, S], actions [N, A] float32 -> out [N, 2] (Q1 | Q2).  Reads the
    parameter tensors in place, so a Polyak update by `target_param.data.copy_` is seen by the next
    call.  supported(critic): both nets Linear-ReLU stacks of equal shape, hidden 128/256/512, <= 8
    hidden layers, S + A <= 16, contiguous float32 parameters on the device, 16-byte aligned."""

    def __init__(self, critic):
        self.critic = critic
        self.lib = L.load()
        self.params = []
        for net in (critic.q1, critic.q2):
            hidden, last, _ = _q_linears(net)
            self.params.append([t for m in hidden + [last] for t in (m.weight, m.bias)])
        hidden = _q_linears(critic.q1)[0]
        self.D, self.H, self.nl = hidden[0].in_features, hidden[0].out_features, len(hidden)
        self._ptrs = tuple((C.c_void_p * len(p))() for p in self.params)

    @staticmethod
    def supported(critic):
        shapes = []
        for net in (critic.q1, critic.q2):
            hidden, last, ok = _q_linears(net)
            if not ok or len(hidden) > 8:
                return False
            H = hidden[0].out_features
            ps = [p for m in hidden + [last] for p in (m.weight, m.bias)]
            if not (H in (128, 256, 512) and 2 <= hidden[0].in_features <= 16 and last.out_features == 1
                    and last.in_features == H and all(m.in_features == H and m.out_features == H for m in hidden[1:])
                    and all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and p.data_ptr() % 16 == 0
                            for p in ps)):
                return False
            shapes.append((hidden[0].in_features, H, len(hidden)))
        return shapes[0] == shapes[1]

    def ptrs(self):
        """(params_q1, params_q2) as pd_sac_critic / pd_sac_td_target take them (read now)."""
        for arr, ps in zip(self._ptrs, self.params):
            for k, t in enumerate(ps):
                arr[k] = t.data_ptr()
        return self._ptrs

    def __call__(self, states, actions, out):
        S, A = int(states.shape[1]), int(actions.shape[1])
        if S + A != self.D:
            raise ValueError(f"state_dim + action_dim = {S + A}, the critic takes {self.D}")
        p1, p2 = self.ptrs()
        L.check(self.lib.pd_sac_critic(int(states.shape[0]), S, A, self.H, self.nl, _ptr(states), _ptr(actions), p1, p2,
                                       _ptr(out), _stream(states.device)))
        return out


_TAG_TD_EPS = 64                  # kTagTdEps (csrc/pd_common.h)
_TAG_ACT_EPS = 72                 # kTagActEps


def td_eps(seed, draw, batch, action_dim, device, tag=_TAG_TD_EPS):
    """pd_sac_td_target's eps draws [batch, A] as torch expressions (the fallback's eps source):
    the same Philox4x32-10 blocks and the same Box-Muller in binary64 (torch's log, cos and sin in
    place of the kernel's), cast to float32 -- the kernel's values to float32 rounding.  tag: the
    Philox purpose tag (pd_sac_actor_grad's draws: _TAG_ACT_EPS)."""
    i64 = dict(dtype=torch.int64, device=device)
    mask = 0xFFFFFFFF
    pairs = (action_dim + 1) // 2
    row = torch.arange(batch, **i64)[:, None].expand(batch, pairs)
    c = [row & mask, torch.full_like(row, draw & mask), torch.full_like(row, (draw >> 32) & mask),
         (tag + torch.arange(pairs, **i64))[None, :].expand(batch, pairs)]
    k0, k1 = seed & mask, (seed >> 32) & mask
    for _ in range(10):                                    # (int64 products wrap: the low 64 bits are exact)
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [((p1 >> 32) & mask) ^ c[1] ^ k0, p1 & mask, ((p0 >> 32) & mask) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & mask, (k1 + 0xBB67AE85) & mask

    def u01(hi, lo):
        return ((hi >> 5).double() * 67108864.0 + (lo >> 6).double()) * (1.0 / 9007199254740992.0)

    u1, u2 = 1.0 - u01(c[0], c[1]), u01(c[2], c[3])
    rho = torch.sqrt(-2.0 * torch.log(u1))
    ang = 6.283185307179586 * u2
    z = torch.stack([rho * torch.cos(ang), rho * torch.sin(ang)], dim=2).reshape(batch, 2 * pairs)
    return z[:, :action_dim].float().contiguous()


class TdTarget:
    """The torch.no_grad() block of SACPyTorch.update (sac_pytorch.py:439-443) as one launch,
    pd_sac_td_target: actor.sample(next_states), critic_target(next_states, next_actions),
    min(q1, q2) - alpha * log_prob and rewards + (1 - dones) * gamma * next_q, from the [B, W] rows
    behind a buffer's sample (`buffer.last_rows`: state | action | reward | next_state | done).
    log_alpha is the learner's device tensor: the kernel reads it, so the temperature the optimizer
    just stepped is used without a host read; the nets' parameters are read in place (a Polyak
    `copy_` into the target critic is seen by the next call).  No host synchronisation.

    __call__(rows, out=None, draw=None, eps=None, next_actions=None, next_log_prob=None, next_q=None,
    heads=None, eps_out=None) -> target_q [B, 1] (`out`, [B] or [B, 1] float32, when given; else a
    tensor the object owns per batch size, overwritten by the next call).  eps [B, A]: the rsample
    noise; None: drawn in the kernel from (seed, draw, row, component), draw defaulting to a counter
    that advances by one per call.  The optional outputs receive the intermediate values.
    Where supported() is false (a net outside the kernels' shapes) the same block is evaluated with
    torch on the same eps source (td_eps), so callers need no branch."""

    def __init__(self, actor, critic_target, log_alpha, gamma, seed=0):
        self.actor, self.critic, self.log_alpha = actor, critic_target, log_alpha
        self.gamma, self.seed = float(gamma), int(seed)
        self.draws = 0
        self._out = {}
        self.kernel = self.supported(actor, critic_target, log_alpha)
        if self.kernel:
            self.lib = L.load()
            self.ak, self.ck = ActorKernel(actor), CriticKernel(critic_target)

    @staticmethod
    def supported(actor, critic, log_alpha):
        if not (ActorKernel.supported(actor) and CriticKernel.supported(critic)):
            return False
        S, A = actor.shared_net[0].in_features, actor.mean.out_features
        return (critic.q1[0].in_features == S + A and log_alpha.dtype == torch.float32 and log_alpha.is_cuda
                and log_alpha.numel() == 1)

    def ptrs(self):
        """(actor_params, params_q1, params_q2) as pd_sac_td_target takes them."""
        return (self.ak.ptrs(),) + tuple(self.ck.ptrs())

    @torch.no_grad()
    def _torch(self, rows, eps, outs):
        a = self.actor
        S, A = a.shared_net[0].in_features, a.mean.out_features
        reward, ns, done = rows[:, S + A:S + A + 1], rows[:, S + A + 1:2 * S + A + 1], rows[:, 2 * S + A + 1:]
        f = a.shared_net(ns)
        mean, raw = a.mean(f), a.log_std(f)
        ls = torch.clamp(raw, a.log_std_min, a.log_std_max)
        sd = ls.exp()
        x = mean + sd * eps
        act = torch.tanh(x)
        lp = (-((x - mean) ** 2) / (2 * sd ** 2) - ls - 0.9189385332046727
              - torch.log(1 - act.pow(2) + 1e-6)).sum(-1, keepdim=True)
        na = act * a.max_action
        q1, q2 = self.critic(ns, na)
        next_q = torch.min(q1, q2) - self.log_alpha.detach().exp() * lp
        target = reward + (1 - done) * self.gamma * next_q
        for name, v in (("next_actions", na), ("next_log_prob", lp), ("next_q", torch.cat([q1, q2], dim=1)),
                        ("heads", torch.cat([mean, raw], dim=1)), ("eps_out", eps)):
            if outs[name] is not None:
                outs[name].copy_(v.reshape(outs[name].shape))
        return target

    def __call__(self, rows, out=None, draw=None, eps=None, next_actions=None, next_log_prob=None, next_q=None,
                 heads=None, eps_out=None):
        B = int(rows.shape[0])
        if eps is None:
            if draw is None:
                draw = self.draws
                self.draws += 1
            draw = int(draw) & (2 ** 64 - 1)
        outs = dict(next_actions=next_actions, next_log_prob=next_log_prob, next_q=next_q, heads=heads, eps_out=eps_out)
        if out is None:
            out = self._out.get(B)
            if out is None:
                out = self._out[B] = torch.empty(B, 1, dtype=torch.float32, device=rows.device)
        if not self.kernel:
            A = self.actor.mean.out_features
            e = eps if eps is not None else td_eps(self.seed & (2 ** 64 - 1), draw, B, A, rows.device)
            out.copy_(self._torch(rows, e, outs).reshape(out.shape))
            return out.reshape(B, 1)
        for t in (rows, out, eps) + tuple(outs.values()):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("TdTarget: contiguous float32 tensors are required")
        a, ak, ck = self.actor, self.ak, self.ck
        pa, p1, p2 = self.ptrs()
        L.check(self.lib.pd_sac_td_target(B, ak.S, ak.A, _ptr(rows), int(rows.shape[1]), ak.H, ak.nl, pa,
                                          a.log_std_min, a.log_std_max, a.max_action, ck.H, ck.nl, p1, p2,
                                          _ptr(self.log_alpha), self.gamma, self.seed & (2 ** 64 - 1),
                                          0 if eps is not None else draw, _ptr(eps), _ptr(out), _ptr(next_actions),
                                          _ptr(next_log_prob), _ptr(next_q), _ptr(heads), _ptr(eps_out),
                                          _stream(rows.device)))
        return out.reshape(B, 1)


def _adam_reasons(optimizer, params):
    """Why pd_adam_step does not take this optimizer over exactly `params`: a list of words, empty
    for a plain torch.optim.Adam with one param group -- "adam", "param_groups", "params",
    "weight_decay", "amsgrad", "maximize", "capturable", "fused", "differentiable", "lr"."""
    if type(optimizer) is not torch.optim.Adam:
        return ["adam"]
    if len(optimizer.param_groups) != 1:
        return ["param_groups"]
    why = []
    g = optimizer.param_groups[0]
    if len(params) > L.ADAM_MAX_TENSORS or len(g["params"]) != len(params) or not all(
            a is b for a, b in zip(g["params"], params)):
        why.append("params")
    if g.get("weight_decay", 0) != 0:
        why.append("weight_decay")
    why += [k for k in ("amsgrad", "maximize", "capturable", "fused", "differentiable") if g.get(k)]
    if isinstance(g["lr"], torch.Tensor):
        why.append("lr")
    return why


def _adam_ensure_state(optimizer, params):
    """torch.optim.Adam's state of `params`, created if empty (as Adam._init_group does), `step` a
    host tensor."""
    st = optimizer.state
    for p in params:
        s = st[p]
        if len(s) == 0:
            s["step"] = torch.tensor(0.0, dtype=torch.float32)
            s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        elif s["step"].is_cuda:
            s["step"] = s["step"].cpu()


def _adam_advance(optimizer, params):
    """Advance every tensor's `step` (a host tensor: no device work); (step_size, bc2_sqrt, beta1,
    beta2, eps) as pd_adam_step takes them, from param_groups as they are now."""
    st, g = optimizer.state, optimizer.param_groups[0]
    for p in params:
        st[p]["step"] += 1
    t = int(st[params[0]]["step"].item())
    beta1, beta2 = g["betas"]
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    return float(g["lr"]) / bc1, bc2 ** 0.5, beta1, beta2, float(g["eps"])


class CriticUpdate:
    """The critic step of SACPyTorch.update as three launches and no host synchronisation
    (csrc/pdsacupd.hip): critic(states, actions), the loss of sac_pytorch.py:457-468 (MSE or L1, with
    or without PER weights), zero_grad() + backward() (pd_sac_critic_grad: the gradients land in
    p.grad, overwritten), then clip_grad_norm_, critic_optimizer.step() and the Polyak loop of step
    8 (pd_adam_step), and the |td| of step 7 that buffer.update_priorities takes.

    optimizer: the caller's torch.optim.Adam over critic.parameters().  Its state -- exp_avg,
    exp_avg_sq, step -- is created if empty and then used in place, so optimizer.state_dict() and
    load_state_dict() keep working and torch's own step() may continue from it; lr, betas and eps are
    read from param_groups at each call; `step` (a host tensor) is advanced on the host.

    td_abs = upd(rows, target_q, weights=None): rows [B, >= S + A] float32 with unit column stride
    (state | action first: buffer.last_rows, or a packed [B, S + A]), target_q [B] or [B, 1] (TdTarget's
    output), weights [B] or [B, 1] or None.  Returns td_abs [B]; upd.q [B, 2], upd.critic_loss [1] and
    upd.grad_norm [1] (None without max_grad_norm) are device tensors -- reading them is the caller's
    synchronisation.  All four are owned by the object per batch size and overwritten by the next call.
    upd.backward(rows, target_q, weights=None, dq=None) runs the forward and backward passes only
    (for another optimizer); dq [B, 2] replaces the loss's own gradient dLoss/dq.

    Where supported() is false -- a net outside the kernels' shapes, or an optimizer that is not a
    plain Adam (weight decay, amsgrad, maximize, capturable / fused, several param groups) -- the same
    steps run in torch (autograd, clip_grad_norm_, optimizer.step(), the Polyak
    loop) and return the same things."""

    def __init__(self, critic, critic_target, optimizer, tau=0.005, use_l1_loss=False, max_grad_norm=None):
        self.critic, self.critic_target, self.optimizer = critic, critic_target, optimizer
        self.tau, self.use_l1_loss = float(tau), bool(use_l1_loss)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.kernel = self.supported(critic, optimizer, critic_target)
        self.q = self.critic_loss = self.grad_norm = None
        self._out = {}
        hidden = _q_linears(critic.q1)[0]
        self.D = hidden[0].in_features
        if self.kernel:
            self.lib = L.load()
            self.ck, self.tk = CriticKernel(critic), CriticKernel(critic_target)
            self.params = self.ck.params[0] + self.ck.params[1]
            self.targets = self.tk.params[0] + self.tk.params[1]
            n, vp = len(self.params), C.c_void_p
            half = n // 2
            self._g = ((vp * half)(), (vp * half)())
            self._lists = tuple((vp * n)() for _ in range(5))      # params, grads, exp_avg, exp_avg_sq, targets
            self._numel = (C.c_int64 * n)(*[p.numel() for p in self.params])
            H, nl = self.ck.H, self.ck.nl
            self.n_partials = 2 * (H // 64 + (nl - 1) * (H // 16) * (H // 128) + H // 128)
            self._np = C.c_int32(0)

    @staticmethod
    def reasons(critic, optimizer, critic_target=None):
        """Why the kernel path does not take this critic and optimizer: a list of words, empty when
        supported -- "shape" (not two Linear-ReLU stacks of equal shape with hidden 128 / 256 / 512,
        <= 8 hidden layers and S + A <= 16), "tensors" (parameters not contiguous float32 on the
        device, 16-byte aligned), "target" (critic_target of other shapes), and the optimizer's:
        "adam", "param_groups", "params", "weight_decay", "amsgrad", "maximize", "capturable", "fused",
        "differentiable", "lr"."""
        why = []
        nets = [getattr(critic, "q1", None), getattr(critic, "q2", None)]
        shapes = []
        for net in nets:
            hidden, last, ok = _q_linears(net) if isinstance(net, nn.Sequential) else ([], None, False)
            if not ok or len(hidden) > 8:
                shapes.append(None)
                continue
            H = hidden[0].out_features
            good = (H in (128, 256, 512) and 2 <= hidden[0].in_features <= 16 and last.out_features == 1
                    and last.in_features == H and all(m.in_features == H and m.out_features == H for m in hidden[1:]))
            shapes.append((hidden[0].in_features, H, len(hidden)) if good else None)
        if None in shapes or shapes[0] != shapes[1]:
            why.append("shape")
        params = list(critic.parameters())
        if not all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and p.data_ptr() % 16 == 0
                   for p in params):
            why.append("tensors")
        if critic_target is not None:
            tp = list(critic_target.parameters())
            if ([tuple(p.shape) for p in tp] != [tuple(p.shape) for p in params]
                    or [n for n, _ in critic_target.named_parameters()] != [n for n, _ in critic.named_parameters()]):
                why.append("target")
            elif "tensors" not in why and not CriticKernel.supported(critic_target):
                why.append("target")
        return why + _adam_reasons(optimizer, params)

    @staticmethod
    def supported(critic, optimizer, critic_target=None):
        return not CriticUpdate.reasons(critic, optimizer, critic_target)

    # ---- the torch path
    def _loss(self, q1, q2, t, w):
        f = F.l1_loss if self.use_l1_loss else F.mse_loss
        if w is not None:
            return (w * f(q1, t, reduction="none") + w * f(q2, t, reduction="none")).mean()
        return f(q1, t) + f(q2, t)

    def _torch_backward(self, rows, target_q, weights, dq):
        B = int(rows.shape[0])
        sa = rows[:, :self.D]
        q1, q2 = self.critic.q1(sa), self.critic.q2(sa)
        t = None if target_q is None else target_q.detach().reshape(B, 1)
        w = None if weights is None else weights.detach().reshape(B, 1)
        self.optimizer.zero_grad()
        loss = None if t is None else self._loss(q1, q2, t, w)
        if dq is not None:
            torch.autograd.backward([q1, q2], [dq[:, :1], dq[:, 1:]])
        else:
            loss.backward()
        self.q = torch.cat([q1, q2], dim=1).detach()
        self.critic_loss = None if loss is None else loss.detach().reshape(1)
        if t is None:
            return None
        return torch.max((t - q1).abs(), (t - q2).abs()).detach().reshape(B)

    def _torch_step(self):
        self.grad_norm = None
        if self.max_grad_norm is not None:
            self.grad_norm = torch.nn.utils.clip_grad_norm_(self.critic.parameters(),
                                                            max_norm=self.max_grad_norm).reshape(1)
        self.optimizer.step()
        with torch.no_grad():
            for p, tp in zip(self.critic.parameters(), self.critic_target.parameters()):
                tp.data.copy_((1 - self.tau) * tp.data + self.tau * p.data)

    # ---- the kernel path
    def _buffers(self, B, dev):
        out = self._out.get(B)
        if out is None:
            nbytes = int(self.lib.pd_sac_critic_grad_scratch_bytes(B, self.ck.H, self.ck.nl))
            f32 = dict(dtype=torch.float32, device=dev)
            out = dict(q=torch.empty(B, 2, **f32), td_abs=torch.empty(B, **f32), loss=torch.empty(1, **f32),
                       grad_norm=torch.empty(1, **f32), partials=torch.empty(self.n_partials, **f32),
                       scratch=torch.empty((nbytes + 3) // 4, **f32))
            self._out[B] = out
        return out

    def _grad_ptrs(self):
        half = len(self.params) // 2
        for k, p in enumerate(self.params):
            if p.grad is None or not (p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self._g[k // half][k % half] = p.grad.data_ptr()
        return self._g

    def _kernel_backward(self, rows, target_q, weights, dq):
        B = int(rows.shape[0])
        for t in (target_q, weights, dq):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() in (B, 2 * B)):
                raise ValueError("CriticUpdate: contiguous float32 tensors of the batch's length are required")
        if not (rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] >= self.D
                and (B == 0 or rows.stride(1) == 1)):
            raise ValueError("CriticUpdate: rows [B, >= S + A] float32 with unit column stride are required")
        o = self._buffers(B, rows.device)
        p1, p2 = self.ck.ptrs()
        g1, g2 = self._grad_ptrs()
        self._np.value = self.n_partials
        want = target_q is not None
        L.check(self.lib.pd_sac_critic_grad(B, self.D - 1, 1, self.ck.H, self.ck.nl, _ptr(rows),
                                            int(rows.stride(0)) if B else self.D, _ptr(target_q), _ptr(weights),
                                            L.SAC_LOSS_L1 if self.use_l1_loss else L.SAC_LOSS_L2, _ptr(dq), p1, p2, g1, g2,
                                            _ptr(o["q"]), _ptr(o["td_abs"]) if want else None, None,
                                            _ptr(o["loss"]) if want else None, _ptr(o["partials"]), C.byref(self._np),
                                            _ptr(o["scratch"]), o["scratch"].numel() * 4, _stream(rows.device)))
        self.q, self.critic_loss = o["q"], (o["loss"] if want else None)
        return o["td_abs"] if want else None

    def _kernel_step(self, B, dev):
        _adam_ensure_state(self.optimizer, self.params)
        step_size, bc2_sqrt, beta1, beta2, eps = _adam_advance(self.optimizer, self.params)
        st = self.optimizer.state
        lp, lg, lm, lv, lt = self._lists
        for k, (p, tp) in enumerate(zip(self.params, self.targets)):
            s = st[p]
            lp[k], lg[k], lt[k] = p.data_ptr(), p.grad.data_ptr(), tp.data_ptr()
            lm[k], lv[k] = s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()
        o = self._buffers(B, dev)
        clip = self.max_grad_norm is not None
        L.check(self.lib.pd_adam_step(len(self.params), lp, lg, lm, lv, self._numel, lt, step_size, bc2_sqrt, beta1,
                                      beta2, eps, self.max_grad_norm if clip else 0.0, _ptr(o["partials"]),
                                      self.n_partials, _ptr(o["grad_norm"]), self.tau, _stream(dev)))
        self.grad_norm = o["grad_norm"] if clip else None

    def backward(self, rows, target_q, weights=None, dq=None):
        """The forward and backward passes alone: the gradients in p.grad (overwritten), q and
        critic_loss set; returns td_abs [B] (None without target_q)."""
        if not self.kernel:
            return self._torch_backward(rows, target_q, weights, dq)
        return self._kernel_backward(rows, target_q, weights, dq)

    def __call__(self, rows, target_q, weights=None):
        td_abs = self.backward(rows, target_q, weights)
        if int(rows.shape[0]) == 0:
            return td_abs
        if self.kernel:
            self._kernel_step(int(rows.shape[0]), rows.device)
        else:
            self._torch_step()
        return td_abs


def _actor_shape(actor):
    """(S, A, H, hidden layer count) of an Actor inside pd_sac_actor's shapes, else None."""
    net = getattr(actor, "shared_net", None)
    if not isinstance(net, nn.Sequential) or not isinstance(getattr(actor, "mean", None), nn.Linear) \
            or not isinstance(getattr(actor, "log_std", None), nn.Linear):
        return None
    lins = [m for m in net if isinstance(m, nn.Linear)]
    acts = [m for m in net if not isinstance(m, nn.Linear)]
    if not lins or len(lins) > 8 or len(acts) != len(lins) or any(not isinstance(m, nn.ReLU) for m in acts):
        return None
    S, H, A = lins[0].in_features, lins[0].out_features, actor.mean.out_features
    ok = (H in (128, 256, 512) and S <= 16 and A <= 8 and all(m.in_features == H and m.out_features == H for m in lins[1:])
          and actor.mean.in_features == H and actor.log_std.in_features == H and actor.log_std.out_features == A)
    return (S, A, H, len(lins)) if ok else None


def _actor_dims(actor):
    """(state_dim, action_dim) of an actor, inside pd_sac_actor's shapes or not (the torch path's): the
    first Linear's inputs and the mean head's outputs."""
    sh = _actor_shape(actor)
    if sh is not None:
        return sh[:2]
    first = next((m for m in actor.modules() if isinstance(m, nn.Linear)), None)
    mean = getattr(actor, "mean", None)
    if first is None or not isinstance(mean, nn.Linear):
        raise ValueError("ActorUpdate: an actor with a Linear layer and a Linear `mean` head is required")
    return first.in_features, mean.out_features


def _critic_shape(critic):
    """(S + A, H, hidden layer count) of a twin critic inside pd_sac_critic's shapes, else None."""
    shapes = []
    for net in (getattr(critic, "q1", None), getattr(critic, "q2", None)):
        hidden, last, ok = _q_linears(net) if isinstance(net, nn.Sequential) else ([], None, False)
        if not ok or len(hidden) > 8:
            return None
        H = hidden[0].out_features
        if not (H in (128, 256, 512) and 2 <= hidden[0].in_features <= 16 and last.out_features == 1
                and last.in_features == H and all(m.in_features == H and m.out_features == H for m in hidden[1:])):
            return None
        shapes.append((hidden[0].in_features, H, len(hidden)))
    return shapes[0] if shapes[0] == shapes[1] else None


def _kernel_tensor(p):
    return p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() and p.data_ptr() % 16 == 0


class ActorUpdate:
    """The actor and temperature steps of SACPyTorch.update (sac_pytorch.py:485-521) as five launches
    and no host synchronisation (csrc/pdsacact.hip): actor.sample(states), critic(states, new_actions)
    with the critic as it is now (CriticUpdate has just stepped it), min(q1, q2), the actor loss with or
    without PER weights, zero_grad() + backward() through both Q nets into the actor and the
    temperature loss's gradient (pd_sac_actor_grad: three launches, the gradients land in p.grad,
    overwritten), then clip_grad_norm_ and actor_optimizer.step() (pd_adam_step over the actor's
    tensors) and alpha_optimizer.step() (pd_adam_step over the one-element log_alpha).

    actor_optimizer: the caller's torch.optim.Adam over actor.parameters(); alpha_optimizer: the
    caller's torch.optim.Adam over [log_alpha], or None for no entropy tuning (alpha_loss is then 0
    and log_alpha and its .grad are untouched).  Their state is created if empty and then used in
    place, as CriticUpdate does.  log_alpha: a one-element float32 device tensor that requires grad
    (the reference's torch.tensor(np.log(0.2)) is float64: see reasons()).  target_entropy defaults
    to -action_dim (sac_pytorch.py:321).

    log_prob = upd(rows, weights=None, draw=None, eps=None): rows [B, >= S] float32 with unit column
    stride whose first S columns are the state (buffer.last_rows, or packed states), weights [B] or
    [B, 1] or None, eps [B, A] the rsample noise or None: drawn in the kernel from (seed, draw, row,
    component) under a Philox tag of its own (72; TdTarget's is 64, so the same seed and draw give
    independent noise), draw defaulting to a counter that advances by one per call.  Returns log_prob
    [B, 1]; upd.new_actions [B, A], upd.q [B, 2], upd.actor_loss [1], upd.alpha_loss [1] and
    upd.grad_norm [1] (None without max_grad_norm) are device tensors -- reading them is the caller's
    synchronisation.  All are owned by the object per batch size and overwritten by the next call.
    upd.backward(...) runs the forward and backward passes only (for another optimizer); its keyword
    outputs heads, eps_out, dq_da, dheads_out receive the intermediate values, and dheads [B, 2A]
    replaces the upstream gradient dLoss / d(mean | raw log_std) (no critic pass then).

    One difference from the reference: actor_loss.backward() there also accumulates into the critic's
    p.grad and into log_alpha.grad (both are zeroed before their next use).  Here the critic's p.grad
    stays as CriticUpdate left it, and log_alpha.grad holds the temperature loss's gradient.

    Where supported() is false the same steps run in torch (autograd, clip_grad_norm_, the optimizers'
    own step()) on the same eps source and return the same things."""

    def __init__(self, actor, critic, log_alpha, actor_optimizer, alpha_optimizer=None, target_entropy=None,
                 max_grad_norm=None, seed=0):
        self.actor, self.critic, self.log_alpha = actor, critic, log_alpha
        self.actor_optimizer, self.alpha_optimizer = actor_optimizer, alpha_optimizer
        self.S, self.A = _actor_dims(actor)
        self.target_entropy = float(-self.A if target_entropy is None else target_entropy)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.seed, self.draws = int(seed), 0
        self.kernel = self.supported(actor, critic, log_alpha, actor_optimizer, alpha_optimizer)
        self.new_actions = self.q = self.actor_loss = self.alpha_loss = self.grad_norm = None
        self._out = {}
        if self.kernel:
            self.lib = L.load()
            self.ak, self.ck = ActorKernel(actor), CriticKernel(critic)
            self.params = list(self.ak.params)
            n, vp = len(self.params), C.c_void_p
            self._g = (vp * n)()
            self._lists = tuple((vp * n)() for _ in range(4))      # params, grads, exp_avg, exp_avg_sq
            self._numel = (C.c_int64 * n)(*[p.numel() for p in self.params])
            self._alpha_lists = tuple((vp * 1)() for _ in range(4))
            self._one = (C.c_int64 * 1)(1)
            H, nl = self.ak.H, self.ak.nl
            self.n_partials = H // 64 + (nl - 1) * (H // 16) * (H // 128) + H // 128
            self._np = C.c_int32(0)

    @staticmethod
    def reasons(actor, critic, log_alpha, actor_optimizer, alpha_optimizer=None):
        """Why the kernel path does not take these: a list of words, empty when supported -- "actor"
        (not pd_sac_actor's shapes: Linear-ReLU stack, hidden 128 / 256 / 512, <= 8 hidden layers, S <=
        16, A <= 8), "critic" (not two Linear-ReLU stacks of equal shape inside pd_sac_critic's, or
        their input is not S + A), "tensors" (a parameter not contiguous float32 on the device, 16-byte
        aligned), "log_alpha" (not a one-element float32 device tensor: the reference's
        torch.tensor(np.log(0.2)) is float64), the actor optimizer's words (CriticUpdate.reasons) and
        the temperature optimizer's with the prefix "alpha_"."""
        why = []
        ash, csh = _actor_shape(actor), _critic_shape(critic)
        if ash is None:
            why.append("actor")
        if csh is None or (ash is not None and csh[0] != ash[0] + ash[1]):
            why.append("critic")
        if not all(_kernel_tensor(p) for p in list(actor.parameters()) + list(critic.parameters())):
            why.append("tensors")
        if not (isinstance(log_alpha, torch.Tensor) and log_alpha.dtype == torch.float32 and log_alpha.is_cuda
                and log_alpha.numel() == 1):
            why.append("log_alpha")
        if ash is not None:
            lins = [m for m in actor.shared_net if isinstance(m, nn.Linear)] + [actor.mean, actor.log_std]
            why += _adam_reasons(actor_optimizer, [t for m in lins for t in (m.weight, m.bias)])
        elif type(actor_optimizer) is not torch.optim.Adam:
            why.append("adam")
        if alpha_optimizer is not None:
            why += ["alpha_" + w for w in _adam_reasons(alpha_optimizer, [log_alpha])]
        return why

    @staticmethod
    def supported(actor, critic, log_alpha, actor_optimizer, alpha_optimizer=None):
        return not ActorUpdate.reasons(actor, critic, log_alpha, actor_optimizer, alpha_optimizer)

    def _draw(self, draw, eps):
        if eps is not None:
            return 0
        if draw is None:
            draw = self.draws
            self.draws += 1
        return int(draw) & (2 ** 64 - 1)

    def _buffers(self, B, dev):
        out = self._out.get(B)
        if out is None:
            f32 = dict(dtype=torch.float32, device=dev)
            out = dict(new_actions=torch.empty(B, self.A, **f32), log_prob=torch.empty(B, 1, **f32),
                       q=torch.empty(B, 2, **f32), actor_loss=torch.zeros(1, **f32), alpha_loss=torch.zeros(1, **f32),
                       grad_norm=torch.empty(1, **f32))
            if self.kernel:
                nbytes = int(self.lib.pd_sac_actor_grad_scratch_bytes(B, self.A, self.ak.H, self.ak.nl))
                out.update(partials=torch.empty(self.n_partials, **f32), scratch=torch.empty((nbytes + 3) // 4, **f32))
            self._out[B] = out
        return out

    # ---- the torch path
    def _torch_backward(self, rows, weights, draw, eps, outs, dheads):
        a, B, S, A = self.actor, int(rows.shape[0]), self.S, self.A
        o = self._buffers(B, rows.device)
        if eps is None:
            eps = td_eps(self.seed & (2 ** 64 - 1), draw, B, A, rows.device, tag=_TAG_ACT_EPS)
        states = rows[:, :S]
        w = None if weights is None else weights.detach().reshape(B, 1)
        if isinstance(getattr(a, "shared_net", None), nn.Module) and isinstance(getattr(a, "log_std", None), nn.Module):
            f = a.shared_net(states)
            mean, raw = a.mean(f), a.log_std(f)
            ls = torch.clamp(raw, a.log_std_min, a.log_std_max)
        else:                      # (an actor of another build: its own forward; `heads` then holds the clamped log_std)
            mean, ls = a(states)
            raw = ls
        sd = ls.exp()
        x = mean + sd * eps
        act = torch.tanh(x)
        lp = (-((x - mean) ** 2) / (2 * sd ** 2) - ls - 0.9189385332046727
              - torch.log(1 - act.pow(2) + 1e-6)).sum(-1, keepdim=True)
        na = act * a.max_action
        params = list(a.parameters())
        self.actor_optimizer.zero_grad()
        got = dict(heads=torch.cat([mean, raw], dim=1), eps_out=eps)
        if dheads is not None:
            grads = torch.autograd.grad([mean, raw], params, [dheads[:, :A], dheads[:, A:]], allow_unused=True)
        else:
            if outs.get("dq_da") is not None:
                na = na.detach().requires_grad_(True)       # (a leaf, for the Q nets' input gradient alone)
                q1, q2 = self.critic(states, na)
                got["dq_da"] = torch.stack([torch.autograd.grad(q1.sum(), na, retain_graph=True)[0],
                                            torch.autograd.grad(q2.sum(), na)[0]], dim=1)
                na = act * a.max_action
            q1, q2 = self.critic(states, na)
            alpha = self.log_alpha.detach().exp()
            t = alpha * lp - torch.min(q1, q2)
            loss = (t if w is None else w * t).mean()
            heads_g = torch.autograd.grad(loss, [mean, raw], retain_graph=True)
            got["dheads_out"] = torch.cat(heads_g, dim=1)
            grads = torch.autograd.grad(loss, params, allow_unused=True)
            o["q"].copy_(torch.cat([q1, q2], dim=1).detach())
            o["actor_loss"].copy_(loss.detach().reshape(1))
        for p, g in zip(params, grads):
            p.grad = torch.zeros_like(p) if g is None else g.detach().to(p.dtype)
        if self.alpha_optimizer is not None:
            t = (lp + self.target_entropy).detach()
            g = -(t if w is None else w * t).mean()
            self.log_alpha.grad = g.to(self.log_alpha.dtype).reshape(self.log_alpha.shape)
            o["alpha_loss"].copy_((self.log_alpha.detach().reshape(()) * g).reshape(1))
        o["new_actions"].copy_(na.detach())
        o["log_prob"].copy_(lp.detach())
        for name, v in got.items():
            if outs.get(name) is not None:
                outs[name].copy_(v.detach().reshape(outs[name].shape))

    def _torch_step(self):
        self.grad_norm = None
        if self.max_grad_norm is not None:
            self.grad_norm = torch.nn.utils.clip_grad_norm_(self.actor.parameters(),
                                                            max_norm=self.max_grad_norm).reshape(1)
        self.actor_optimizer.step()
        if self.alpha_optimizer is not None:
            self.alpha_optimizer.step()

    # ---- the kernel path
    def _grad_ptrs(self):
        for k, p in enumerate(self.params):
            if p.grad is None or not (p.grad.is_contiguous() and p.grad.dtype == torch.float32):
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self._g[k] = p.grad.data_ptr()
        return self._g

    def _kernel_backward(self, rows, weights, draw, eps, outs, dheads):
        B = int(rows.shape[0])
        for t, cols in ((weights, 1), (eps, self.A), (dheads, 2 * self.A), (outs.get("heads"), 2 * self.A),
                        (outs.get("eps_out"), self.A), (outs.get("dq_da"), 2 * self.A),
                        (outs.get("dheads_out"), 2 * self.A)):
            if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == B * cols):
                raise ValueError("ActorUpdate: contiguous float32 tensors of the batch's length are required")
        if not (rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[1] >= self.S
                and (B == 0 or rows.stride(1) == 1)):
            raise ValueError("ActorUpdate: rows [B, >= S] float32 with unit column stride are required")
        o = self._buffers(B, rows.device)
        a, ak, ck = self.actor, self.ak, self.ck
        p1, p2 = ck.ptrs()
        self._np.value = self.n_partials
        tune = self.alpha_optimizer is not None
        la = self.log_alpha
        if tune and (la.grad is None or la.grad.dtype != torch.float32):
            la.grad = torch.zeros_like(la)
        L.check(self.lib.pd_sac_actor_grad(
            B, ak.S, ak.A, _ptr(rows), int(rows.stride(0)) if B else ak.S, _ptr(weights), ak.H, ak.nl, ak.ptrs(),
            self._grad_ptrs(), a.log_std_min, a.log_std_max, a.max_action, ck.H, ck.nl, p1, p2, _ptr(la),
            self.target_entropy, self.seed & (2 ** 64 - 1), draw, _ptr(eps), _ptr(dheads), _ptr(o["new_actions"]),
            _ptr(o["log_prob"]), _ptr(o["q"]), _ptr(outs.get("heads")), _ptr(outs.get("eps_out")),
            _ptr(outs.get("dq_da")), _ptr(outs.get("dheads_out")), _ptr(o["actor_loss"]),
            _ptr(o["alpha_loss"]) if tune else None, _ptr(la.grad) if tune else None, _ptr(o["partials"]),
            C.byref(self._np), _ptr(o["scratch"]), o["scratch"].numel() * 4, _stream(rows.device)))

    def _kernel_step(self, B, dev):
        o = self._buffers(B, dev)
        clip = self.max_grad_norm is not None
        opt = self.actor_optimizer
        _adam_ensure_state(opt, self.params)
        step_size, bc2_sqrt, beta1, beta2, eps = _adam_advance(opt, self.params)
        lp, lg, lm, lv = self._lists
        for k, p in enumerate(self.params):
            s = opt.state[p]
            lp[k], lg[k] = p.data_ptr(), p.grad.data_ptr()
            lm[k], lv[k] = s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()
        L.check(self.lib.pd_adam_step(len(self.params), lp, lg, lm, lv, self._numel, None, step_size, bc2_sqrt, beta1,
                                      beta2, eps, self.max_grad_norm if clip else 0.0, _ptr(o["partials"]),
                                      self.n_partials, _ptr(o["grad_norm"]), 0.0, _stream(dev)))
        self.grad_norm = o["grad_norm"] if clip else None
        opt = self.alpha_optimizer
        if opt is not None:
            la = self.log_alpha
            _adam_ensure_state(opt, [la])
            step_size, bc2_sqrt, beta1, beta2, eps = _adam_advance(opt, [la])
            s = opt.state[la]
            lp, lg, lm, lv = self._alpha_lists
            lp[0], lg[0], lm[0], lv[0] = la.data_ptr(), la.grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()
            L.check(self.lib.pd_adam_step(1, lp, lg, lm, lv, self._one, None, step_size, bc2_sqrt, beta1, beta2, eps, 0.0,
                                          None, 0, None, 0.0, _stream(dev)))

    def backward(self, rows, weights=None, draw=None, eps=None, dheads=None, heads=None, eps_out=None, dq_da=None,
                 dheads_out=None):
        """The forward and backward passes alone: the actor's gradients in p.grad (overwritten),
        log_alpha.grad set (with an alpha_optimizer), new_actions, q, actor_loss and alpha_loss set;
        returns log_prob [B, 1]."""
        B = int(rows.shape[0])
        draw = self._draw(draw, eps)
        outs = dict(heads=heads, eps_out=eps_out, dq_da=dq_da, dheads_out=dheads_out)
        if self.kernel:
            self._kernel_backward(rows, weights, draw, eps, outs, dheads)
        else:
            self._torch_backward(rows, weights, draw, eps, outs, dheads)
        o = self._buffers(B, rows.device)
        self.new_actions, self.q, self.actor_loss, self.alpha_loss = o["new_actions"], o["q"], o["actor_loss"], o["alpha_loss"]
        return o["log_prob"]

    def __call__(self, rows, weights=None, draw=None, eps=None):
        log_prob = self.backward(rows, weights, draw, eps)
        if int(rows.shape[0]) == 0:
            return log_prob
        if self.kernel:
            self._kernel_step(int(rows.shape[0]), rows.device)
        else:
            self._torch_step()
        return log_prob


STAT_NAMES = ("step",
              "state_mean", "state_min", "state_max", "state_std", "state_kurtosis",
              "action_mean", "action_min", "action_max", "action_std", "action_kurtosis",
              "reward_mean", "reward_min", "reward_max", "reward_std", "reward_kurtosis",
              "critic_loss", "actor_loss", "alpha_loss", "alpha_value",
              "q_value_mean", "q_value_min", "q_value_max", "q_value_std",
              "log_prob_mean", "log_prob_min", "log_prob_max", "log_prob_std",
              "target_q_mean", "target_q_min", "target_q_max", "target_q_std",
              "per_beta", "per_mean_weight", "per_max_priority",
              "actor_grad_norm", "critic_grad_norm")      # pd_sac_stat_name, sac_pytorch.py:346-397
_PER_STATS = STAT_NAMES[32:35]
_GRAD_STATS = STAT_NAMES[35:37]
assert len(STAT_NAMES) == L.SAC_N_STATS


class LearningStats:
    """The reference's learning_stats (sac_pytorch.py:346-397) and _track_learning_stats (:553-634) on
    the device: a [capacity, 37] float64 ring of rows in the reference's key order (STAT_NAMES), each
    written by ONE pd_sac_learning_stats launch from the tensors a learner update leaves behind --
    nothing is read back until the ring is full, or flush(), to_dict(), save_csv() or a read of
    .columns / .rows asks for it, and then the filled rows come over in one copy.

    record(rows, td_target_out, critic_update, actor_update, log_prob, weights, buffer): rows the
    sampled [B, W] rows (buffer.last_rows), td_target_out TdTarget's [B, 1], log_prob ActorUpdate's
    return value, weights [B, 1] or None; it reads critic_update.critic_loss / .grad_norm,
    actor_update.q / .actor_loss / .alpha_loss / .grad_norm / .log_alpha and, where the buffer has
    them, buffer.max_prio_dev and buffer.beta.  The `step` column is the object's own counter (.step,
    0 at first, as the reference's self.updates).  A column whose input is missing is NaN.

    kernel=None (default): the kernel where the inputs are contiguous float32 device tensors inside its
    domain (S <= 16, A <= 8, B <= 65536), else the torch path; kernel=False: always the torch path --
    the same 37 numbers by float64 torch reductions on the device tensors, stacked into the row
    without an .item(); kernel=True: the kernel or an error.

    to_dict() -> {name: list} in column order, without the PER keys and the grad-norm keys when they
    were never given (the reference has them only under use_per / clip_gradients).  save_csv(path)
    appends the rows not yet saved, with a header only when the file does not exist
    (save_learning_stats, sac_pytorch.py:636-684)."""

    def __init__(self, state_dim, action_dim, device, capacity=1024, kernel=None):
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.device = torch.device(device)
        self.capacity = max(1, int(capacity))
        self.kernel = kernel
        self.buf = torch.zeros(self.capacity, L.SAC_N_STATS, dtype=torch.float64, device=self.device)
        self.step = 0                 # the next row's `step`
        self.n = 0                    # rows recorded
        self.last_kernel = None       # whether the last record() went through the kernel
        self._flushed = 0             # rows copied to the host
        self._saved = 0               # rows written by save_csv
        self._host = []               # [k, 37] arrays, in order
        self.has_per = self.has_grad_norms = False
        self.lib = None

    # ---- recording
    def _kernel_ok(self, B, tensors, scalars):
        if not (self.device.type == "cuda" and 1 <= B <= L.SAC_STATS_MAX_BATCH and self.state_dim <= 16
                and self.action_dim <= 8):
            return False
        for t, numel in tensors:
            if t is not None and not (t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == numel):
                return False
        return all(t is None or (t.dtype == torch.float32 and t.is_cuda and t.numel() == 1) for t in scalars)

    @staticmethod
    def _series(x):
        """[5, k] mean, min, max, std (ddof 0), kurtosis (Fisher, biased) of the k columns of x [n, k]
        in binary64, two-pass; torch's min and max give NaN for a column that holds one."""
        n = x.shape[0]
        mean = x.sum(0) / n
        d2 = (x - mean) ** 2
        m2, m4 = d2.sum(0) / n, (d2 * d2).sum(0) / n
        return torch.stack([mean, x.min(0).values, x.max(0).values, m2.sqrt(), m4 / (m2 * m2) - 3.0])

    @torch.no_grad()
    def _torch_row(self, rows, q, target_q, log_prob, weights, scalars, log_alpha, per_beta, out):
        S, A, f64 = self.state_dim, self.action_dim, torch.float64
        B = int(rows.shape[0])
        dev = rows.device

        def const(v):
            return torch.full((1,), float(v), dtype=f64, device=dev)

        def scalar(t):
            return const("nan") if t is None else t.detach().reshape(-1)[:1].to(f64)

        def flat(t, cols=4):
            return self._series(t.detach().reshape(B, -1)[:, :1].to(f64))[:cols, 0]

        closs, aloss, alloss, maxp, agn, cgn = scalars
        per_dim = self._series(rows[:, :S].to(f64))
        state = per_dim[:, 0]
        for d in range(1, S):         # (ascending, as the kernel adds them: torch's sum has its own order)
            state = state + per_dim[:, d]
        state = state / S
        action = self._series(rows[:, S:S + A].to(f64).reshape(-1, 1))[:, 0]
        qq = q.detach().reshape(B, 2)
        qmin = torch.fmin(qq[:, 0], qq[:, 1])
        alpha = log_alpha.detach().reshape(-1)[:1].float().exp().to(f64)
        have_w = weights is not None
        out.copy_(torch.cat([
            const(self.step), state, action, flat(rows[:, S + A:S + A + 1], 5),
            scalar(closs), scalar(aloss), scalar(alloss), alpha,
            flat(qmin), flat(log_prob), flat(target_q),
            const(per_beta if have_w else "nan"),
            weights.detach().reshape(-1).to(f64).sum().reshape(1) / B if have_w else const("nan"), scalar(maxp),
            scalar(agn), scalar(cgn)]))

    def record(self, rows, td_target_out, critic_update, actor_update, log_prob, weights=None, buffer=None):
        B, S, A = int(rows.shape[0]), self.state_dim, self.action_dim
        q, log_alpha = actor_update.q, actor_update.log_alpha
        scalars = (critic_update.critic_loss, actor_update.actor_loss, actor_update.alpha_loss,
                   getattr(buffer, "max_prio_dev", None) if weights is not None else None,
                   actor_update.grad_norm, critic_update.grad_norm)
        per_beta = float(getattr(buffer, "beta", float("nan")))
        out = self.buf[self.n % self.capacity]
        use = self.kernel
        if use is None or use:
            ok = (rows.dim() == 2 and rows.dtype == torch.float32 and rows.is_cuda and B > 0 and rows.stride(1) == 1
                  and rows.stride(0) >= S + A + 1
                  and self._kernel_ok(B, ((q, 2 * B), (td_target_out, B), (log_prob, B), (weights, B)),
                                      scalars + (log_alpha,)))
            if use and not ok:
                raise ValueError("LearningStats(kernel=True): contiguous float32 device tensors inside "
                                 "pd_sac_learning_stats' domain are required")
            use = ok
        if use:
            if self.lib is None:
                self.lib = L.load()
            L.check(self.lib.pd_sac_learning_stats(
                B, S, A, _ptr(rows), int(rows.stride(0)), _ptr(q), _ptr(td_target_out), _ptr(log_prob), _ptr(weights),
                *[_ptr(t) for t in scalars[:3]], _ptr(log_alpha), *[_ptr(t) for t in scalars[3:]], per_beta,
                int(self.step), _ptr(out), _stream(rows.device)))
        else:
            self._torch_row(rows, q, td_target_out, log_prob, weights, scalars, log_alpha, per_beta, out)
        self.last_kernel = bool(use)
        self.has_per = self.has_per or weights is not None
        self.has_grad_norms = self.has_grad_norms or scalars[4] is not None or scalars[5] is not None
        self.step += 1
        self.n += 1
        if self.n - self._flushed >= self.capacity:
            self.flush()

    # ---- reading
    def flush(self):
        """The rows recorded since the last flush to the host, in ONE copy (the reader's
        synchronisation)."""
        k = self.n - self._flushed
        if k <= 0:
            return
        a = self._flushed % self.capacity
        b = a + k
        if b <= self.capacity:
            part = self.buf[a:b]
        else:                          # (wrapped: gathered on the device, still one copy)
            part = torch.cat([self.buf[a:], self.buf[:b - self.capacity]])
        self._host.append(part.cpu().numpy().copy())
        self._flushed = self.n

    @property
    def rows(self):
        """[n, 37] float64 numpy: every row recorded so far."""
        import numpy as np
        self.flush()
        if len(self._host) > 1:
            self._host = [np.concatenate(self._host)]
        return self._host[0] if self._host else np.zeros((0, L.SAC_N_STATS))

    @property
    def columns(self):
        """{name: [n] float64 numpy} over all 37 columns."""
        r = self.rows
        return {name: r[:, k] for k, name in enumerate(STAT_NAMES)}

    def keys(self):
        return [n for n in STAT_NAMES if (self.has_per or n not in _PER_STATS)
                and (self.has_grad_norms or n not in _GRAD_STATS)]

    def to_dict(self, start=0):
        cols = self.columns
        out = {name: cols[name][start:].tolist() for name in self.keys()}
        out["step"] = [int(v) for v in out["step"]]
        return out

    def __len__(self):
        return self.n

    def save_csv(self, path):
        """Append the rows not yet saved to `path`; the header only when the file does not exist.
        Returns the number of rows written."""
        import os
        new = self.to_dict(start=self._saved)
        k = len(new["step"])
        if k == 0:
            return 0
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        exists = os.path.isfile(path)
        try:
            import pandas as pd
        except ImportError:
            pd = None
        if pd is not None:
            pd.DataFrame(new).to_csv(path, mode="a" if exists else "w", header=not exists, index=False)
        else:
            import csv
            with open(path, "a" if exists else "w", newline="") as f:
                w = csv.writer(f)
                if not exists:
                    w.writerow(list(new))
                w.writerows(zip(*new.values()))
        self._saved = self.n
        return k


def sac_update(buffer, td_target, critic_update, actor_update, batch_size, stats=None):
    """One learner update in the order of SACPyTorch.update (sac_pytorch.py:411-531): sample, TdTarget,
    CriticUpdate, ActorUpdate, update_priorities (a prioritized buffer; a uniform DeviceReplayBuffer,
    whose sample is a 5-tuple, has no weights and no priorities) and, with `stats` (a LearningStats),
    the update's learning_stats row (step 9) -- after update_priorities, so that it logs what the
    reference logs: alpha after its step, the max priority after step 7, beta after the sample's
    annealing.  With a KernelPrioritizedReplayBuffer and the objects on their kernel paths this is a
    fixed sequence of launches on device pointers: nothing is read back and nothing is returned."""
    batch = buffer.sample(batch_size)
    weights, indices = (batch[5], batch[6]) if len(batch) >= 7 else (None, None)
    rows = buffer.last_rows
    target_q = td_target(rows)
    td_abs = critic_update(rows, target_q, weights)
    log_prob = actor_update(rows, weights)
    if indices is not None:
        buffer.update_priorities(indices, td_abs)
    if stats is not None:
        stats.record(rows, target_q, critic_update, actor_update, log_prob, weights, buffer)


class SACCollector:
    """One collection step of N envs on this rank: actor -> env step -> transition rows -> (gather)
    -> learner-rank buffer.  `obs` always holds the observation the actor sees next (the
    post-auto-reset observation of envs whose episode ended).

    fused=True (default): ONE launch per step where the actor fits the kernel (ActorKernel
    shapes; pd_step_sac_fused): the reference Actor's MLP and both heads for each workgroup's 16
    envs in the step kernel's prologue (MFMA hidden layers, activations in LDS), then the action
    sampled from the heads (eps drawn there, Philox; torch.randn's role), the env step, and the
    transition rows written by the kernel epilogue straight into the learner's replay ring at the
    ring's device-held position, with the new rows' priorities set to the buffer's max priority;
    the next float32 observation into `obs`.  (Handles that do not step 16 lanes per env: the
    actor as its own launch, pd_sac_actor, the same bits.)  Actor shapes the kernel does not
    cover: PyTorch's shared_net and one GEMM over both heads, then pd_step_sac_ring.  On several
    ranks the rows go to a local slab instead and `all_gather_into_tensor` (RCCL) appends them
    on the learner rank.
    fused=False: Actor.sample, pd_step, transition_slab, pd_observe, buffer.add_batch (the unfused
    reference path, eps from torch.randn with `generator`).
    use_graph=True captures the step into one HIP graph (the ring position lives on the device, so
    replays append in order).  Off by default: on ROCm 7 each replay of the one-kernel graph left
    an 8.6 us gap before its step kernel, where eager launches from a host that keeps ahead of
    the GPU run back to back (c5: 0.0434 against 0.0392 ms per step, profiles/r05_exp_c5_graph.jsonl).  The gather runs eagerly after
    each replay.  flush_every > 0: a pd_flush_misses call every that many steps (0, the default:
    none -- the step launch inserts the neighbourhoods it solved itself, ABI 10).
    step() returns the step's transition rows: a view of the replay ring's rows (valid until the
    ring wraps onto them) in ring mode, else a fresh tensor.
    collect(k) is k steps in one call (pd_collect_sac: the actor inside the step kernel's fused-step
    loop, the span between two learner updates, during which the actor is fixed), the same bits
    as k step() calls; step() and collect() may alternate.  use_graph applies to step() only."""

    def __init__(self, env, actor, buffer=None, dist=None, learner_rank=0, generator=None,
                 deterministic=False, use_graph=False, flush_every=0, fused=True):
        self.env, self.actor, self.buffer, self.dist = env, actor, buffer, dist
        self.learner_rank, self.generator, self.deterministic = learner_rank, generator, deterministic
        self.rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
        self.multi = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
        self.obs = env.reset().float().contiguous()
        self.flush_every = flush_every
        self.steps = 0
        self.graph = None
        self.use_graph = use_graph
        self.fused = fused
        S, A = env.obs_dim, env.action_dim
        dev = self.obs.device
        self._slab_buf = torch.empty(env.n, 2 * S + A + 2, dtype=torch.float32, device=dev)
        self.action = torch.empty(env.n, A, dtype=torch.float32, device=dev)
        self.heads = torch.empty(env.n, 2 * A, dtype=torch.float32, device=dev)
        self.eps_out = None           # [N, A] to receive the kernel's eps draws (tests)
        self.heads_out = None         # [N, 2A] to receive the actor's heads (tests)
        self.kernel = ActorKernel(actor) if fused and ActorKernel.supported(actor) else None
        H = actor.mean.in_features
        self._head_w = torch.empty(2 * A, H, dtype=torch.float32, device=dev)
        self._head_b = torch.empty(2 * A, dtype=torch.float32, device=dev)
        # ring mode: this process holds the buffer and steps every env of the job
        self.ring = fused and buffer is not None and not self.multi and buffer.capacity >= env.n

    def _heads(self):
        if self.kernel is not None:
            return self.kernel(self.obs, self.heads)
        # (shapes pd_sac_actor does not cover) torch's MLP and one GEMM over both heads, the
        # head weights copied on every step (inside a captured graph too: never stale)
        a = self.actor
        torch.cat([a.mean.weight, a.log_std.weight], out=self._head_w)
        torch.cat([a.mean.bias, a.log_std.bias], out=self._head_b)
        f = a.shared_net(self.obs)
        return torch.addmm(self._head_b, f, self._head_w.t(), out=self.heads)

    def _body(self):
        """actor -> env step -> transition rows and next obs into self.obs (no syncs); returns
        the local slab, or None when the rows went straight into the replay ring."""
        if self.fused:
            a = self.actor
            kw = dict(deterministic=self.deterministic, action=self.action, obs32=self.obs, eps_out=self.eps_out)
            if self.ring:
                b = self.buffer
                kw.update(ring=b.data, capacity=b.capacity, ring_state=b.state_dev,
                          priorities=getattr(b, "priorities", None), max_priority=getattr(b, "max_prio_dev", None))
            else:
                kw.update(ring=self._slab_buf)
            if self.kernel is not None:
                k = self.kernel
                self.env.step_sac_fused(k.S, k.A, k.H, k.nl, k.ptrs(), a.log_std_min, a.log_std_max, a.max_action,
                                        heads=self.heads_out, **kw)
            else:
                self.env.step_sac_ring(self._heads(), a.log_std_min, a.log_std_max, a.max_action, **kw)
            return None if self.ring else self._slab_buf
        gen = None if self.use_graph else self.generator
        act, _ = self.actor.sample(self.obs, deterministic=self.deterministic, generator=gen, with_log_prob=False)
        act = act.float().contiguous()
        self.env.step_raw_noflush(act)
        slab = transition_slab(self.obs, act, self.env.reward_buf, self.env.obs_buf, self.env.done_buf)
        self.obs.copy_(self.env.observe_raw())                 # copy_ casts: one kernel
        return slab

    def _finish(self, slab):
        self.steps += 1
        if self.flush_every and self.steps % self.flush_every == 0:
            self.env.flush()
        if slab is None:                                       # ring mode: the rows are in place
            start = self.buffer.position
            self.buffer.note_appended(self.env.n)
            return self.buffer.rows(start, self.env.n)
        full = gather_slabs(slab, self.dist)
        if self.rank == self.learner_rank and self.buffer is not None:
            self.buffer.add_batch(full)
        return full.clone() if full is self._slab_buf else full

    @torch.no_grad()
    def step(self):
        if not self.use_graph:
            return self._finish(self._body())
        if self.graph is None:
            # one eager step on a side stream warms the allocator and the kernels; it is a real
            # step (its transitions are kept), then the next step is captured and replayed
            s = torch.cuda.Stream(device=self.obs.device)
            s.wait_stream(torch.cuda.current_stream(self.obs.device))
            with torch.cuda.stream(s):
                slab = self._body()
            torch.cuda.current_stream(self.obs.device).wait_stream(s)
            full = self._finish(slab)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._slab = self._body()
            return full
        self.graph.replay()
        return self._finish(self._slab)

    def _step_logged(self, t, outs):
        """One step() whose reward, done, truncated and trunc_id (handle precision) go to row t of
        the given tensors: the unfused path's pd_step leaves them in the handle's buffers; the
        fused calls return the reward only as the row's float32, so the handle is put back
        (checkpoint, stream-ordered) and pd_step of the step's action gives them, ending in the same
        state (as _evaluate_per_step does)."""
        env = self.env
        if self.fused:
            blob = env.checkpoint()
            rows = self.step()
            env.restore(blob)
            env.step_raw_noflush(self.action)
        else:
            rows = self.step()
        for out, buf in zip(outs, (env.reward_buf, env.done_buf, env.trunc_buf, env.trunc_id_buf)):
            if out is not None:
                out[t].copy_(buf)
        return rows

    @torch.no_grad()
    def collect(self, k, rewards=None, done=None, truncated=None, trunc_id=None):
        """k collection steps of every env; returns the k * N (times the world size) transition
        rows it appended, in step order: a view of the ring's rows in ring mode (unless they
        wrap), else a fresh tensor.  One pd_collect_sac call where the library takes it -- a single
        rank with a buffer writes the ring in place, several ranks write a local [k, N, W] slab,
        all-gather it and append it in step-major order (step_major) -- and k step() calls, the
        same values, where it answers PD_ERR_UNSUPPORTED (a handle that does not step 16 lanes per
        env, hidden 512), for an actor ActorKernel does not cover, with fused=False, and in ring
        mode when k * N rows do not fit the buffer.  rewards [k, N] (handle precision), done /
        truncated [k, N] uint8 and trunc_id [k, N] int8, when given, receive every step's values.
        `obs` is left at the next observation.
        Cost of the fallback with any of these four outputs given and fused=True: the fused step
        calls return the reward only as the row's float32, so every step saves a checkpoint, steps,
        restores it and steps again through pd_step -- two handle copies and a second env step per
        step, more than twice a plain step().  Without the outputs the fallback is k plain step()
        calls."""
        k = int(k)
        env, b = self.env, self.buffer
        outs = (rewards, done, truncated, trunc_id)
        world = self.dist.get_world_size() if self.multi else 1
        rows = None
        # (the choice of path must be the same on every rank: only ring mode, a single rank, looks at
        # the buffer)
        if self.fused and self.kernel is not None and k > 0 and (not self.ring or k * env.n <= b.capacity):
            a = self.actor
            kw = dict(deterministic=self.deterministic, obs32=self.obs, reward=rewards, done=done, truncated=truncated,
                      trunc_id=trunc_id)
            slab = None
            if self.ring:
                kw.update(ring=b.data, capacity=b.capacity, ring_state=b.state_dev,
                          priorities=getattr(b, "priorities", None), max_priority=getattr(b, "max_prio_dev", None))
            else:
                slab = torch.empty(k, env.n, 2 * env.obs_dim + env.action_dim + 2, dtype=torch.float32, device=self.obs.device)
                kw.update(ring=slab)
            try:
                env.collect_sac(self.kernel, k, **kw)
            except L.PdError as err:   # (nothing was launched: the per-step loop below)
                if getattr(err, "status", None) != L.PD_ERR_UNSUPPORTED:
                    raise
            else:
                if self.ring:
                    start = b.position
                    b.note_appended(k * env.n)
                    rows = b.rows(start, k * env.n)
                else:
                    if self.multi:
                        full = torch.empty((world,) + tuple(slab.shape), dtype=slab.dtype, device=slab.device)
                        self.dist.all_gather_into_tensor(full, slab)
                        rows = step_major(full)
                    else:
                        rows = slab.reshape(k * env.n, slab.shape[2])
                    if self.rank == self.learner_rank and b is not None:
                        # (more rows than the buffer holds: step by step, as k step() calls append)
                        per = rows.shape[0] if rows.shape[0] <= b.capacity else world * env.n
                        for r0 in range(0, rows.shape[0], per):
                            b.add_batch(rows[r0:r0 + per])
                before, self.steps = self.steps, self.steps + k
                if self.flush_every and self.steps // self.flush_every != before // self.flush_every:
                    env.flush()
                return rows
        W = 2 * env.obs_dim + env.action_dim + 2
        if k <= 0:
            return torch.empty(0, W, dtype=torch.float32, device=self.obs.device)
        # (ring mode: a step's rows are a view the ring may wrap onto before the loop ends)
        keep = (lambda r: r.clone()) if self.ring else (lambda r: r)
        if all(o is None for o in outs):
            return torch.cat([keep(self.step()) for _ in range(k)])
        return torch.cat([keep(self._step_logged(t, outs)) for t in range(k)])


# ---------------------------------------------------------------------------- evaluation rollouts
class EvalResult(tuple):
    """evaluate_agent's result.  Unpacks like the driver's pair -- `eval_reward, success_rate =
    evaluate_agent(...)[:2]` -- and carries, as attributes, the per-env tensors `returns`, `steps`,
    `done`, `trunc_id` (device), the `trunc_hist` dict {truncation id: episodes} and, with traces,
    `actions` [T, N, A] float32 and `rewards` [T, N] (rows past an env's length: NaN); `fused`
    tells which path ran."""

    def __new__(cls, mean_reward, success_rate, returns, steps, done, trunc_id, trunc_hist, actions=None,
                rewards=None, fused=False):
        self = super().__new__(cls, (mean_reward, success_rate, returns, steps, done, trunc_id, trunc_hist,
                                     actions, rewards))
        self.fused = fused
        return self

    mean_reward = property(lambda s: s[0])
    success_rate = property(lambda s: s[1])
    returns = property(lambda s: s[2])
    steps = property(lambda s: s[3])
    done = property(lambda s: s[4])
    trunc_id = property(lambda s: s[5])
    trunc_hist = property(lambda s: s[6])
    actions = property(lambda s: s[7])
    rewards = property(lambda s: s[8])


def summarize_rollout(returns, done, trunc_id):
    """(mean_reward, success_rate, trunc_hist) of a batch of episodes, one per env: the mean of the
    returns (np.mean(eval_rewards)), the share of episodes whose terminal step had done (the
    driver's success_count / num_episodes, sac_pytorch_powered_descent.py:234-251; a terminal step
    with done AND a truncation id counts as a success, as there) and {truncation id: episodes}
    over every id that occurs (0: none).  Works on CPU and device tensors; the sums run on the
    CPU in binary64."""
    r = returns.detach().to("cpu", torch.float64).reshape(-1)
    d = done.detach().to("cpu").reshape(-1) != 0
    t = trunc_id.detach().to("cpu", torch.int64).reshape(-1)
    n = r.numel()
    if n == 0:
        return float("nan"), float("nan"), {}
    counts = torch.bincount(t.clamp_min(0))
    hist = {int(k): int(c) for k, c in enumerate(counts.tolist()) if c}
    return float(r.sum().item() / n), float(int(d.sum().item()) / n), hist


def _torch_heads(actor, obs, out):
    """[N, 2A] mean | log_std (unclamped) of an actor pd_sac_actor does not cover."""
    f = actor.shared_net(obs)
    return torch.cat([actor.mean(f), actor.log_std(f)], dim=1, out=out)


@torch.no_grad()
def _evaluate_per_step(actor, env, max_steps, deterministic, traces, check_every=16):
    """evaluate_agent on the calls of the collection path, one step at a time: pd_step_sac_fused
    (or the actor and pd_step_sac_ring) gives the step's float32 action and the next float32
    observation; the handle is put back (checkpoint, stream-ordered, no sync) and pd_step of that
    action gives the step's reward, done, truncated and trunc_id in the handle's precision -- the
    SAC step calls return the reward only as the replay row's float32.  Bookkeeping of each env's
    first episode in device tensors; the live count is read back every check_every steps."""
    lib, dev, N, A, S = env.lib, env.device, env.n, env.action_dim, env.obs_dim
    kernel = ActorKernel(actor) if ActorKernel.supported(actor) else None
    obs = env.reset().float().contiguous()
    kw = dict(device=dev)
    act = torch.empty(N, A, dtype=torch.float32, **kw)
    heads = torch.empty(N, 2 * A, dtype=torch.float32, **kw)
    slab = torch.empty(N, 2 * S + A + 2, dtype=torch.float32, **kw)
    blob = torch.empty(int(lib.pd_checkpoint_size(env.h)), dtype=torch.uint8, **kw)
    ret = torch.zeros(N, dtype=env.dtype, **kw)
    steps = torch.zeros(N, dtype=torch.int32, **kw)
    done = torch.zeros(N, dtype=torch.uint8, **kw)
    tid = env.episode_counters()[2].clone()
    live = torch.ones(N, dtype=torch.bool, **kw)
    T = int(max_steps)
    actions = torch.full((T, N, A), float("nan"), dtype=torch.float32, **kw) if traces else None
    rewards = torch.full((T, N), float("nan"), dtype=env.dtype, **kw) if traces else None
    for t in range(T):
        L.check(lib.pd_checkpoint_save(env.h, _ptr(blob), _stream(dev)))
        skw = dict(deterministic=deterministic, ring=slab, action=act, obs32=obs)
        if kernel is not None:
            env.step_sac_fused(kernel.S, kernel.A, kernel.H, kernel.nl, kernel.ptrs(), actor.log_std_min,
                               actor.log_std_max, actor.max_action, **skw)
        else:
            env.step_sac_ring(_torch_heads(actor, obs, heads), actor.log_std_min, actor.log_std_max,
                              actor.max_action, **skw)
        L.check(lib.pd_checkpoint_load(env.h, _ptr(blob), _stream(dev)))
        env.step_raw_noflush(act)
        r = env.reward_buf
        ret = torch.where(live, ret + r, ret)
        steps += live
        if traces:
            actions[t] = torch.where(live[:, None], act, actions[t])
            rewards[t] = torch.where(live, r, rewards[t])
        ended = live & ((env.done_buf | env.trunc_buf) != 0)
        done = torch.where(ended, env.done_buf, done)
        tid = torch.where(live, env.trunc_id_buf, tid)
        live = live & ~ended
        if (t + 1) % check_every == 0 and not bool(live.any()):
            break
    return ret, steps, done, tid, actions, rewards


@torch.no_grad()
def evaluate_agent(actor, env, max_steps=2200, deterministic=True, fused=True, traces=False):
    """The SAC driver's evaluate_agent (sac_pytorch_powered_descent.py:234-251) -- and, with
    traces=True, the loop of visualize_trajectory (:354-376) -- over the handle's N envs, one env
    one episode: every env is reset and driven by actor.sample(state, deterministic) until done or
    truncated (or max_steps).  Returns an EvalResult: (mean_reward, success_rate, ...) with
    success_rate the share of episodes whose terminal step had done.
    fused=True: ONE call, pd_rollout_sac -- the actor inside the step kernel's fused-step loop, no
    host synchronisation -- where the handle steps 16 lanes per env and the actor fits
    (ActorKernel.supported, hidden 128 or 256); otherwise, and with fused=False, the per-step path
    on pd_step_sac_fused / pd_step_sac_ring.  Both paths return the same values."""
    T = int(max_steps)
    out = None
    if fused and ActorKernel.supported(actor) and actor.mean.in_features != 512:
        kw = dict(device=env.device)
        actions = torch.full((T, env.n, env.action_dim), float("nan"), dtype=torch.float32, **kw) if traces else None
        rewards = torch.full((T, env.n), float("nan"), dtype=env.dtype, **kw) if traces else None
        try:
            out = env.rollout_sac(ActorKernel(actor), deterministic=deterministic, reset=True, max_steps=T,
                                  actions_out=actions, rewards_out=rewards) + (actions, rewards)
        except L.PdError as err:   # (a handle the kernel refuses: not 16 lanes per env)
            if getattr(err, "status", None) != L.PD_ERR_UNSUPPORTED:
                raise
    used_fused = out is not None
    if out is None:
        out = _evaluate_per_step(actor, env, T, deterministic, traces)
    ret, steps, done, tid, actions, rewards = out
    mean_reward, success_rate, hist = summarize_rollout(ret, done, tid)
    return EvalResult(mean_reward, success_rate, ret, steps, done, tid, hist, actions, rewards, fused=used_fused)
