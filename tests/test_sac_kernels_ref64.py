"""tests/sac_kernels_ref64.py pinned without a GPU: its restatements of the SAC kernels against fp64 torch autograd,
torch.optim.Adam and SAC.store_torch, and the conditions the inputs of tests/test_sac_kernels_gpu.py have to satisfy (clamp
edges, saturated actions, ties, the episode-history wrap)."""
import collections
import math

import numpy as np
import pytest
import torch

import sac_kernels_ref64 as ref
from kernel_helpers import normals
from sac_helpers import BanditEnv

SEED, CTR = 0x5AC1EA12, 7
T = lambda x: torch.as_tensor(np.asarray(x, np.float64))
close = lambda a, b: np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=1e-7, atol=1e-9)


def test_draws_are_the_normals_of_the_kernel_helpers():
    for rows, A in ((1, 1), (7, 2), (300, 23)):
        eps, deps = ref.draws(SEED, rows, CTR, A)
        assert np.array_equal(eps, normals(SEED, rows, CTR, A))
        assert eps.shape == deps.shape == (rows, A) and bool((deps >= 0).all()) and float(deps.max()) < 1e-5


@pytest.mark.parametrize("B,A", [(1, 1), (110, 1), (40, 23), (300, 28)])
def test_head_fwd_and_bwd_against_autograd(B, A):
    """log pi and dhead of tanh(mu + exp(clamp(log_std)) eps) with SB3's correction; dL/da is a random linear function of a, log pi
    enters with alpha / B.  The rows hold every clamp edge (torch.clamp passes the gradient at the edge itself, as SB3's)."""
    head = ref.head_rows(B, A)
    st = np.zeros(16, np.float32)
    st[0] = math.log(0.2)
    v, _ = ref.head_fwd(head, B, B, A, SEED, CTR, st, 0, -float(A), 3e-4)
    K, col = A + 5, 5
    dx = np.random.default_rng(B + A).standard_normal((2 * B, K)).astype(np.float32)
    alpha = float(np.float32(0.2))
    g, _ = ref.head_bwd(head, B, A, SEED, CTR, dx, K, col, alpha)
    h = T(head).requires_grad_(True)
    eps = T(normals(SEED, B, CTR, A))
    ls = h[:, A:].clamp(-20.0, 2.0)
    a = torch.tanh(h[:, :A] + ls.exp() * eps)
    logp = (-0.5 * eps ** 2 - ls - ref.LOG_SQRT_2PI).sum(1) - torch.log(1 - a ** 2 + 1e-6).sum(1)
    assert close(v["a"], a.detach()) and close(v["logp"], logp.detach())
    da = T(dx)[:B, col:] + T(dx)[B:, col:]
    ((da * a).sum() + alpha / B * logp.sum()).backward()
    assert close(g["dhead"], h.grad) and close(g["dbias"], h.grad.sum(0))
    lsr = head[:, A:]
    assert bool((g["dhead"][:, A:][(lsr < -20) | (lsr > 2)] == 0).all())
    assert bool((g["dhead"][:, A:][(lsr == -20) | (lsr == 2)] != 0).all())
    assert close(v["st"][8], float(logp.detach().mean())) and close(v["st"][5], -math.log(0.2) * float(logp.detach().mean() - A))
    assert close(v["st"][4], 0.2)


@pytest.mark.parametrize("B", [1, 7, 257])
def test_loss_heads_against_autograd(B):
    I = ref.loss_inputs(B, ties=False)
    assert not bool((I["qpi"][0] == I["qpi"][1]).any()) and not bool((I["qt"][0] == I["qt"][1]).any())
    alpha, gamma = float(np.float32(0.2)), float(np.float32(0.99))
    v, _ = ref.critic_loss(I["q"], I["qt"], I["logp_next"], I["rew"], I["done"], B, gamma, alpha)
    q = T(I["q"]).requires_grad_(True)
    y = T(I["rew"]) + (1 - T(I["done"])) * gamma * (T(I["qt"]).min(0).values - alpha * T(I["logp_next"]))
    loss = 0.5 * sum(torch.nn.functional.mse_loss(q[i], y) for i in range(2))
    loss.backward()
    assert close(v["dq"], q.grad) and close(v["db3"], q.grad.sum(1)) and close(v["loss"], float(loss.detach()))
    v, _ = ref.actor_loss(I["qpi"], I["logp"], B, alpha)
    q = T(I["qpi"]).requires_grad_(True)
    loss = (alpha * T(I["logp"]) - torch.min(q, dim=0).values).mean()
    loss.backward()
    assert np.allclose(v["dq"], q.grad.numpy(), rtol=1e-7, atol=0) and close(v["loss"], float(loss.detach()))


def test_actor_loss_ties_go_to_the_first_critic_as_torch_min():
    I = ref.loss_inputs(9)
    v, _ = ref.actor_loss(I["qpi"], I["logp"], 9, 0.2)
    q = T(I["qpi"].T.copy()).requires_grad_(True)                    # [B, 2]: torch.min over dim 1 takes the first on a tie
    torch.min(q, dim=1).values.sum().backward()
    assert np.array_equal(v["dq"] != 0, q.grad.numpy().T != 0)
    assert bool((v["dq"][0, ::3] != 0).all()) and bool((v["dq"][1, ::3] == 0).all())


def test_adam_scalar_against_torch_adam():
    p = torch.nn.Parameter(torch.tensor([-1.6], dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=3e-4)
    state, got = (-1.6, 0.0, 0.0, 0.0), {}
    for t, g in enumerate([3.0, -40.0, 0.5, 7.0, -2.0], 1):
        p.grad = torch.tensor([g], dtype=torch.float64)
        opt.step()
        state, bound = ref.adam_scalar(*state, g, 0.0, 3e-4, 0.9, 0.999, 1e-8)
        got[t] = (state[0], float(p.detach()))
        assert state[3] == t and all(b >= 0 for b in bound)
    for t in (1, 5):
        assert abs(got[t][0] - got[t][1]) < 1e-14, (t, got[t])


@pytest.mark.parametrize("nets", [1, 2])
def test_linear_relu_and_its_backward_against_torch(nets):
    B, O, I, ldx = 9, 6 * nets, 5, 7
    rng = np.random.default_rng(nets)
    X, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((B, ldx), (O, I), (O,)))
    v, d = ref.linear_relu(X, ldx, W, b, B, O, I, nets)
    x = T(X[:, :I]).requires_grad_(True)
    Wt, bt = T(W).requires_grad_(True), T(b).requires_grad_(True)
    y = torch.relu(x @ Wt.T + bt)                                     # [B, O]; net n owns columns [n On, (n + 1) On)
    On = O // nets
    want = y.detach().reshape(B, nets, On).permute(1, 0, 2)
    assert close(v["Y"], want) and v["Y"].shape == d["Y"].shape == (nets, B, On)
    dY = rng.standard_normal((nets, B, On)).astype(np.float32)
    y.backward(T(dY).permute(1, 0, 2).reshape(B, O))
    z, _ = ref.relu_bwd_colsum(dY, v["Y"].astype(np.float32), B, On, nets)
    assert close(z["db"].reshape(-1), bt.grad)
    assert close(np.einsum("nbo,bi->noi", z["dZ"].astype(np.float64), X[:, :I].astype(np.float64)).reshape(O, I), Wt.grad)


def test_relu_mask_treats_both_zeros_as_off():
    dY, Y, kind = ref.relu_inputs(5, 3, 1)
    z, _ = ref.relu_bwd_colsum(dY, Y, 5, 3, 1)
    assert bool((z["dZ"][kind <= 1] == 0).all()) and np.array_equal(z["dZ"][kind == 2], dY[kind == 2])
    assert bool(np.signbit(Y[kind == 1]).all()) and float(ref.TINY) > 0


def test_store_against_store_torch():
    from deepmimic_mujoco_amd.sac import SAC
    N, D, A, cap = 5, 6, 3, 3
    env = BanditEnv(N, D, A, seed=1)
    sac = SAC(env, net_arch=(8, 8), buffer_size=cap * N, seed=0, device="cpu")
    assert sac.cap_steps == cap
    last = np.random.default_rng(0).standard_normal((N, D)).astype(np.float32)
    S = ref.new_store_state(N, D, A, cap, last)
    for step in range(7):
        I = ref.store_inputs(N, D, A, step)
        sac.store_torch(torch.as_tensor(S["last_obs"]), torch.as_tensor(I["act"]), {k: torch.as_tensor(I[k]) for k in
                                                                                   ("rew", "done", "obs", "terminal_obs")})
        ref.store(S, N, D, A, cap, **I)
        for k, name in (("obs", "r_obs"), ("act", "r_act"), ("rew", "r_rew"), ("done", "r_done"), ("next_obs", "r_next")):
            assert np.array_equal(sac.ring[k].numpy(), S[name]), (step, k)
        assert np.array_equal(sac.ep_acc.numpy(), S["ep_acc"])
        assert sac.ring_state.tolist()[:2] == S["ring"][:2].tolist() and S["counter"] == step + 1
    assert [e for s in S["episodes"] for e in s] == list(sac._ep_deque) and S["ring"][3] == len(sac._ep_deque) > 0


# ---- the conditions the GPU tests' inputs have to satisfy
@pytest.mark.parametrize("R,A", [(255, 1), (257, 1), (600, 1), (513, 2), (255, 23), (300, 28)])
def test_head_rows_hold_the_edges(R, A):
    head = ref.head_rows(R, A)
    mu, ls = head[:, :A], head[:, A:]
    assert set(np.unique(mu)) == set(ref.MU_SET.tolist()) and set(np.unique(ls)) == set(ref.LS_SET.tolist())
    for edge in (-20.0, 2.0):
        assert int((ls == np.float32(edge)).sum()) >= 8
        assert int((ls == np.nextafter(np.float32(edge), np.float32(0))).sum()) >= 8
        assert int((ls == np.nextafter(np.float32(edge), np.float32(10 * edge))).sum()) >= 8
    # |u| > 10: 1 - tanh < 5e-9, far inside the last half ulp below 1 (3e-8), so an fp32 tanh within 2 ulp returns +-1 exactly
    for ctr in (3, 7):
        u = ref._squash(head, A, ref.draws(SEED, R, ctr, A)[0])[4]
        assert int((np.abs(u) > 10).sum()) >= 8


@pytest.mark.parametrize("B", [1, 7, 255, 256, 257, 1000])
def test_loss_inputs_hold_ties_and_both_done_values(B):
    seen = set()
    for flip in (0, 1):
        I = ref.loss_inputs(B, flip)
        ties = int((I["qpi"][0] == I["qpi"][1]).sum())
        assert ties >= max(B // 4, 1) and not bool((I["q"][0] == I["q"][1]).any())
        seen |= set(I["done"].tolist())
        assert B == 1 or set(I["done"].tolist()) == {0.0, 1.0}
    assert seen == {0.0, 1.0}


@pytest.mark.parametrize("B,O,nets", [(3, 65, 2), (100, 96, 2), (257, 300, 1)])
def test_relu_inputs_hold_every_kind_in_every_column_block(B, O, nets):
    _, Y, kind = ref.relu_inputs(B, O, nets)
    for c0 in range(0, O, 64):
        k = kind[:, :, c0:c0 + 64]
        assert all(int((k == i).sum()) >= 1 for i in range(3))


def test_episode_history_case_wraps_by_whole_steps():
    """N = 5, every env done every step, 25 steps: 125 episodes through the 100-entry history.  100 % 5 == 0, so each step fills
    five whole slots and the history is, as a multiset, the episodes of the last 20 steps whatever the order inside a step."""
    N, D, A, cap = 5, 3, 2, 2
    S = ref.new_store_state(N, D, A, cap, np.zeros((N, D), np.float32))
    for step in range(25):
        ref.store(S, N, D, A, cap, **ref.store_inputs(N, D, A, step, all_done=True))
    assert int(S["ring"][3]) == 125
    want = collections.Counter(e for s in S["episodes"][5:] for e in s)
    got = collections.Counter(zip(S["ep_hist"][:100].astype(np.float64).tolist(), S["ep_hist"][100:].astype(np.float64).tolist()))
    assert got == want and len(want) == 100
    assert collections.Counter(e for s in S["episodes"][:5] for e in s) & got == collections.Counter()
