"""pdenv -- MI355X-native vectorised powered-descent environment.

Drop-in for the env hot path of JvanZyl1/PSSO-SAC-for-powered-descent: the physics step,
ISA atmosphere, exact local-RBF aerodynamics, grid fins, wind and the RL/PSO
reward/termination run as HIP kernels in libpdenv.so (C ABI: include/pdenv.h).
"""
from ._lib import PdError, INFO_FIELDS, load  # noqa: F401
from .env import PoweredDescentEnv  # noqa: F401
from .params import Params, load_pack  # noqa: F401
from .sac import (Critic, CriticKernel, KernelPrioritizedReplayBuffer, LearningStats, TdTarget, evaluate_agent,  # noqa: F401
                  summarize_rollout)
from .agent import SACPyTorch  # noqa: F401

__all__ = ["PoweredDescentEnv", "Params", "load_pack", "PdError", "INFO_FIELDS", "load", "evaluate_agent",
           "summarize_rollout", "KernelPrioritizedReplayBuffer", "Critic", "CriticKernel", "TdTarget",
           "LearningStats", "SACPyTorch"]
