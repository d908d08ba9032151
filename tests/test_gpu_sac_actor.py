"""pd_sac_actor (sac_mlp_tile, pd_sac_mlp.h) over its whole declared domain -- S 1..16, A 1..8,
H in {128, 256, 512}, L 1..8 -- against references outside the kernel.

Exact: integer nets (sac_nets.py) whose every partial sum is an integer below 2**24, so that f32
in any summation order gives the bits of the int64 forward pass; the heads must be EQUAL to it.
The fused step kernel and the rollout kernel are tied to pd_sac_actor bit for bit by their own
tests, so this anchors all three.  Which shape reaches which path: sac_nets.SHAPES.

Real-valued: the kernel's error against a binary64 forward pass of the same float32 parameters,
bounded by a multiple of what torch's own two f32 evaluations (GPU and CPU) cost on the same
inputs (REAL_C below)."""
import json
import os
import sys

import numpy as np
import pytest

import sac_nets as sn

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5     # no integer: no head of an integer net equals it
GUARD = 16


@pytest.fixture(scope="module")
def pd():
    import torch
    import pdenv
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return pdenv


_cases = {}


def int_kernel(S, A, H, L):
    """The integer case of a shape (computed once, never modified): its ActorKernel, observations
    [37][S] and reference heads [37][2A] on the device."""
    import torch
    from pdenv.sac import Actor, ActorKernel
    key = (S, A, H, L)
    if key not in _cases:
        params, obs, ref = sn.int_case(S, A, H, L)
        actor = sn.load_actor(Actor(S, A, hidden_dim=H, n_hidden_layers=L), params).cuda()
        assert ActorKernel.supported(actor)
        _cases[key] = (ActorKernel(actor), torch.from_numpy(obs).cuda(), torch.from_numpy(ref).cuda())
    return _cases[key]


def run_guarded(kern, dobs, n):
    """One pd_sac_actor launch over the first n rows of dobs, copied into an [n + 16][S] buffer
    whose 16 rows past n hold NaN; heads [n + 16][2A] with the sentinel in the 16 guard rows.
    Returns (heads[:n], guard rows)."""
    import torch
    heads = torch.full((n + GUARD, 2 * kern.A), SENTINEL, device="cuda")
    obs = torch.full((n + GUARD, dobs.shape[1]), float("nan"), device="cuda")
    obs[:n] = dobs[:n]
    assert bool(torch.isnan(obs[n:]).all()) and bool(torch.isfinite(obs[:n]).all())
    kern(obs[:n], heads[:n])
    torch.cuda.synchronize()
    return heads[:n], heads[n:]


def assert_exact(got, guard, ref, what):
    import torch
    assert bool((guard == SENTINEL).all()), f"{what}: head rows past n were written"
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {ref.numel()} heads differ from the integer reference; "
                             f"first (row, output) {i}: got {float(got[i])}, want {float(ref[i])}")


@pytest.mark.parametrize("S,A,H,L", sn.SHAPES)
def test_integer_net_exact(pd, S, A, H, L):
    """n = 37 (two full tiles and one of five rows): the heads equal the int64 reference (values,
    so +-0 does not matter), the 16 head rows past n keep their sentinel, and the NaN observation
    rows past n reach no output."""
    kern, dobs, ref = int_kernel(S, A, H, L)
    got, guard = run_guarded(kern, dobs, sn.N_EXACT)
    assert_exact(got, guard, ref, (S, A, H, L))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("S,A,H,L", sn.SHAPES_N)
def test_integer_net_exact_batch_sizes(pd, S, A, H, L, n):
    """Batches below, at and just above the 16-env tile: the first n rows of the same case."""
    kern, dobs, ref = int_kernel(S, A, H, L)
    got, guard = run_guarded(kern, dobs, n)
    assert_exact(got, guard, ref[:n], (S, A, H, L, n))


@pytest.mark.parametrize("S,A,H,L", sn.SHAPES_N)
def test_empty_batch_is_ok_and_writes_nothing(pd, S, A, H, L):
    import torch
    from pdenv import _lib
    from pdenv.env import _ptr, _stream
    kern, dobs, _ = int_kernel(S, A, H, L)
    heads = torch.full((GUARD, 2 * A), SENTINEL, device="cuda")
    st = kern.lib.pd_sac_actor(0, S, H, L, A, _ptr(dobs), kern.ptrs(), _ptr(heads), _stream(dobs.device))
    torch.cuda.synchronize()
    assert st == _lib.PD_OK
    assert bool((heads == SENTINEL).all())
    kern(dobs[:0], heads[:0])                                  # (through the wrapper: an empty tensor)
    torch.cuda.synchronize()
    assert bool((heads == SENTINEL).all())


def test_in_place_update_is_seen_by_the_next_call(pd):
    """ActorKernel reads the parameter tensors in place: after negating one hidden weight row and
    adding 1 to a head bias in place, the next call on the SAME ActorKernel gives the new integer
    reference (the net stays an integer net with the same bound on its partial sums)."""
    import torch
    from pdenv.sac import Actor, ActorKernel
    S, A, H, L = 8, 3, 256, 2
    params, obs, ref = sn.int_case(S, A, H, L, seed=1)
    actor = sn.load_actor(Actor(S, A, hidden_dim=H, n_hidden_layers=L), params).cuda()
    kern = ActorKernel(actor)
    dobs = torch.from_numpy(obs).cuda()
    got, guard = run_guarded(kern, dobs, sn.N_EXACT)
    assert_exact(got, guard, torch.from_numpy(ref).cuda(), "before the update")
    row = 77
    ptrs_before = list(kern.ptrs())
    with torch.no_grad():
        actor.shared_net[2].weight[row].neg_()
        actor.log_std.bias[1] += 1
    assert list(kern.ptrs()) == ptrs_before                    # in place: the same addresses
    new = [p.copy() for p in params]
    new[2][row] = -new[2][row]
    new[2 * L + 3][1] += 1
    ref2, abs_sum, _ = sn.forward(new, obs)
    assert abs_sum < sn.EXACT_LIMIT
    ref2 = ref2.astype(np.float32)
    # a condition on the inputs: the update changes heads of both kinds
    assert (ref2[:, :A] != ref[:, :A]).any() and (ref2[:, A + 1] == ref[:, A + 1] + 1).all()
    got, guard = run_guarded(kern, dobs, sn.N_EXACT)
    assert_exact(got, guard, torch.from_numpy(ref2).cuda(), "after the update")


def test_supported_tells_the_domain(pd):
    """ActorKernel.supported is False for what pd_sac_actor refuses (tests/test_abi.py) and for
    what the wrapper could not hand it: hidden 64, nine hidden layers, S = 17, A = 9, an
    activation other than ReLU, float64 parameters."""
    import torch.nn as nn
    from pdenv.sac import Actor, ActorKernel
    assert ActorKernel.supported(Actor(16, 8, hidden_dim=128, n_hidden_layers=8).cuda())
    assert not ActorKernel.supported(Actor(2, 1, hidden_dim=64).cuda())
    assert not ActorKernel.supported(Actor(2, 1, hidden_dim=128, n_hidden_layers=9).cuda())
    assert not ActorKernel.supported(Actor(17, 1, hidden_dim=128).cuda())
    assert not ActorKernel.supported(Actor(2, 9, hidden_dim=128).cuda())
    tanh = Actor(2, 1, hidden_dim=128).cuda()
    tanh.shared_net[1] = nn.Tanh()
    assert not ActorKernel.supported(tanh)
    assert not ActorKernel.supported(Actor(2, 1, hidden_dim=128).double().cuda())


# ------------------------------------------------------------------ real-valued weights
# err_k <= REAL_C max(err_g, err_c), each error max |. - ref64| over the shape's heads: the kernel
# against what f32 evaluation of the same net in torch's two summation orders costs on the same
# inputs -- not a multiple of anything the kernel produces.  Why 4: the kernel accumulates each
# hidden dot product as ONE chain of H fused multiply-adds, a GEMM library in blocks whose partial
# sums it then adds, so the kernel's random-walk error may sit a small factor (of the order of
# sqrt(H / block)) above torch's, and the maximum over a few hundred heads of either scatters by
# another factor of about 2; an order of magnitude would be a wrong term, not rounding.
# Measured: profiles/sac_actor_shapes.json.
REAL_C = 4.0


def measure_real(S, A, H, L):
    """(err_k, err_g, err_c, max |ref|, live share) of a shape at n = 261."""
    import torch
    from pdenv.sac import ActorKernel
    actor, obs, ref, live = sn.real_case(S, A, H, L)
    with torch.no_grad():
        f = actor.shared_net(obs)
        cpu = torch.cat([actor.mean(f), actor.log_std(f)], dim=1)
        dev = actor.cuda()
        dobs = obs.cuda()
        f = dev.shared_net(dobs)
        gpu = torch.cat([dev.mean(f), dev.log_std(f)], dim=1)
    assert ActorKernel.supported(dev)
    heads = torch.full((sn.N_REAL, 2 * A), float("nan"), device="cuda")
    ActorKernel(dev)(dobs, heads)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(heads).all())
    err = [float((x.cpu().double() - ref).abs().max()) for x in (heads, gpu, cpu)]
    return err[0], err[1], err[2], float(ref.abs().max()), live


@pytest.mark.parametrize("S,A,H,L", sn.SHAPES)
def test_real_net_error_within_torch_f32_error(pd, S, A, H, L):
    err_k, err_g, err_c, top, live = measure_real(S, A, H, L)
    print(f"(S, A, H, L) = {(S, A, H, L)}: err_k {err_k:.3e} err_g {err_g:.3e} err_c {err_c:.3e} "
          f"ratio {err_k / max(err_g, err_c):.2f} max |ref| {top:.3g} live {live:.2f}")
    # conditions on the inputs
    assert 0.1 <= top <= 1e3, top
    assert 0.2 <= live <= 0.8, live
    assert max(err_g, err_c) > 0
    assert err_k <= REAL_C * max(err_g, err_c), (err_k, err_g, err_c)


if __name__ == "__main__":     # python tests/test_gpu_sac_actor.py OUT.json: the measurements alone
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "psso-sac-for-powered-descent_amd"))
    rows = []
    for shape in sn.SHAPES:
        k, g, c, top, live = measure_real(*shape)
        rows.append(dict(shape=list(shape), n=sn.N_REAL, gain=sn.REAL_GAIN, err_k=k, err_g=g, err_c=c,
                         ratio=k / max(g, c), max_abs_ref=top, live=live))
        print(rows[-1])
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(what="pd_sac_actor, torch f32 on the GPU and torch f32 on the CPU against the binary64 "
                            "forward pass of the same float32 parameters: max |. - ref64| over the heads",
                       bound_c=REAL_C, shapes=rows), fh, indent=1)
