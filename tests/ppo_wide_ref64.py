"""fp64 reference of ``dm_ppo_wide_grad`` that rounds where the kernel rounds (test helper, not a conftest).

``csrc/dm_ppo_wide.hip`` multiplies bf16 operands on the matrix pipe with fp32 accumulation and keeps everything else in
fp32.  Its rounding points are few and explicit in the source; this module evaluates the same chain in ``torch.float64``
and applies ``round_fn`` (default: fp64 -> fp32 -> bf16 -> fp64, round to nearest even) exactly there:

* obs -> bf16 (``wide_fwdbwd_kernel``: "observations -> bf16 rows"),
* every weight -> bf16 in the five packed layouts (``wide_pack_kernel``),
* h1 and h2 -> bf16 after tanh (``wide_put4`` in layer 1 / layer 2); tanh' = 1 - h^2 is taken from the ROUNDED h,
* dZ3, dZ2, dZ1 -> bf16 (``wide_f2bf(dz)`` in the loss, ``wide_put4`` in d layer 2, ``wide_store_t4`` in d layer 1),
* the head output (+ bias) and all loss arithmetic stay unrounded.

Plain torch only: nothing of ``deepmimic_mujoco_amd`` is imported and no ``dm_*`` function is called, so a kernel test
compares the project's code with something that shares none of it.  ``ppo_ref64`` supplies the loss of the heads.

BOUNDS at the end of the file holds the error bounds of tests/test_ppo_wide_kernel_gpu.py, per shape and per gradient tensor
/ stage.  UNMEASURED ON THE DEVICE: no MI355X run could be had when they were set, so each is 10 x the distance of this chain
evaluated in fp32 with the kernel's tanh formula from the same chain in fp64 (CPU, worst of the three input seeds SEEDS; floors:
2e-5 for a gradient, the fp32 bound of the loss terms, since its sums over B run in fp32 in another order; one element off by
one bf16 ulp for a stage).  On a device the rule is 4 x the kernel's worst distance
from this reference over the same seeds.  tests/test_ppo_wide_ref64.py relates the bounds to the defect models on the CPU.
"""
import torch

import ppo_ref64 as R

TRUNKS = (("pi", "action_net"), ("vf", "value_net"))       # trunk 0 = policy, 1 = value (DmPpoWideStep's order)
BIAS_WGRAD_H1 = 512          # WIDE_BIAS_WGRAD_H1: from this first-layer width up the bias gradients come from the weight-gradient launch
HEAD_TILE = 32               # the head is padded to one 32-wide tile


def round_bf16(x):
    return x.float().to(torch.bfloat16).double()


def identity(x):
    return x


def dp(D):
    """Observation width padded to a multiple of the k-step (16)."""
    return (D + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ fragment order
def frag_index(n, k, K):
    """Element index of (n, k) of a matrix M[N][K] (N % 32 == 0, K % 16 == 0) in the kernel's fragment order (file header of
    dm_ppo_wide.hip): tiles of 32 rows, k-steps of 16, then the 64 lanes' fragments of 8 elements in lane order — lane
    (k >> 3 & 1) * 32 + (n & 31) holds the 8 consecutive k of row n.  Works on ints and on integer tensors."""
    return (((n >> 5) * (K >> 4) + (k >> 4)) * 64 + ((k >> 3) & 1) * 32 + (n & 31)) * 8 + (k & 7)


def unfrag(T, N, K):
    """The first N * K elements of the flat array T, stored in fragment order, as the ordinary matrix [N][K]."""
    n = torch.arange(N, device=T.device)[:, None]
    k = torch.arange(K, device=T.device)[None, :]
    return T.reshape(-1)[frag_index(n, k, K)]


def packed_reference(P_trunk, D, H1, H2, A_t):
    """The five blocks of one trunk's packed weights as ordinary bf16 matrices, in the order of the packed buffer:
    W1 [H1][Dp] | W2 [H2][H1] | W2^T [H1][H2] | W3 [32][H2] | W3^T [H2][32]; zeros where k >= D or the head row / column >= A_t.
    P_trunk = (W1 [H1][D], W2 [H2][H1], W3 [A_t][H2]) in torch layout."""
    W1, W2, W3 = (w.detach().float() for w in P_trunk)
    assert W1.shape == (H1, D) and W2.shape == (H2, H1) and W3.shape == (A_t, H2)
    w1 = torch.zeros(H1, dp(D), device=W1.device)
    w1[:, :D] = W1
    w3 = torch.zeros(HEAD_TILE, H2, device=W1.device)
    w3[:A_t] = W3
    return [m.contiguous().to(torch.bfloat16) for m in (w1, W2, W2.t(), w3, w3.t())]


# ------------------------------------------------------------------------------------------------ the chain
def _forward(P, obs, rnd, tanh=torch.tanh):
    d = P["log_std"].dtype
    xb = rnd(obs.to(d))
    h1s, h2s, outs = [], [], []
    for pre, head in TRUNKS:
        (W1, b1), (W2, b2) = R._layers(P, pre)
        h1 = rnd(tanh(xb @ rnd(W1.detach()).t() + b1.detach()))
        h2 = rnd(tanh(h1 @ rnd(W2.detach()).t() + b2.detach()))
        outs.append(h2 @ rnd(P[head + ".weight"].detach()).t() + P[head + ".bias"].detach())
        h1s.append(h1)
        h2s.append(h2)
    return xb, h1s, h2s, outs


def log_ratio(P, batch, round_fn=None):
    """log pi(a | s) - old_logp per row, from the chain's (rounded) forward pass."""
    obs, act, _, _, old_logp = batch
    with torch.no_grad():
        _, _, _, outs = _forward(P, obs, round_bf16 if round_fn is None else round_fn)
        return R.logp(act, outs[0], P["log_std"].detach()) - old_logp.to(outs[0])


def wide_chain(P, batch, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True, round_fn=None, bias_route=None, tanh=torch.tanh):
    """One minibatch of the wide learner with the kernel's rounding points.  P: name -> fp64 tensor (ppo_ref64.params64),
    batch = (obs, act, adv, ret, old_logp).  Returns (loss, out8, {name: gradient}, intermediates).

    Forward: both trunks with rounded operands (module docstring).  Loss: ppo_ref64.head_loss on the UNROUNDED head outputs,
    autograd through the head only (d loss / d mean, d value, d log_std).  Backward by hand, as the kernel does it:
        dZ3 = round(d loss / d head)                      [B][32], columns >= A (policy) / >= 1 (value) zero
        dZ2 = round((dZ3 round(W3)) * (1 - h2^2))
        dZ1 = round((dZ2 round(W2)) * (1 - h1^2))
        dW3 = dZ3^T h2,  dW2 = dZ2^T h1,  dW1 = dZ1^T round(obs)
    g_log_std = sum_b dlogp_b (z_b^2 - 1) - ent_coef is what autograd gives for the unrounded head (ppo_loss arithmetic, the
    block-0 epilogue of wide_wgrad_kernel subtracts ent_coef).

    Bias gradients follow the kernel's route (bias_route: None = by H1, "wgrad" or "chain"):
    * H1 >= 512 ("wgrad", WIDE_BIAS_WGRAD_H1): all three are column sums of the ROUNDED dZ — wide_wgrad_tile multiplies the
      bf16 dZ^T fragments by a fragment of ones ("accb[p] = mfma(A_[p][i], ones, accb[p])").
    * H1 < 512 ("chain", a.bias_in_chain): gb3 sums the rounded dZ3 ("s += wide_bf2f(... dZ3s ...)" after the loss), but gb2
      and gb1 sum the UNROUNDED fp32 products: "s0 += (v[0] + v[1]) + (v[2] + v[3])" sits beside wide_put4 in d layer 2 and
      "s += (v[0] + v[1]) + (v[2] + v[3])" beside wide_store_t4 in d layer 1, both on the values before they are packed.

    tanh: the activation (the kernel's is 1 - 2 / (1 + exp(2 x)) in fp32; the reference takes torch.tanh).

    intermediates: {"xb": [B][D], "h1": [t], "h2": [t], "dz1": [t], "dz2": [t], "dz3": [t] ([B][32])}, values as rounded."""
    rnd = round_bf16 if round_fn is None else round_fn
    obs, act, adv, ret, old_logp = batch
    with torch.no_grad():
        xb, h1s, h2s, outs = _forward(P, obs, rnd, tanh)
    mean = outs[0].clone().requires_grad_(True)
    value = outs[1].squeeze(-1).clone().requires_grad_(True)
    ls = P["log_std"].detach().clone().requires_grad_(True)
    total, out8 = R.head_loss(mean, ls, value, act, adv, ret, old_logp, clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef,
                              normalize=normalize)
    g_mean, g_value, g_ls = torch.autograd.grad(total, [mean, value, ls])
    H1 = h1s[0].shape[1]
    route = bias_route or ("wgrad" if H1 >= BIAS_WGRAD_H1 else "chain")
    assert route in ("wgrad", "chain")
    grads = {"log_std": g_ls}
    inter = {"xb": xb, "h1": h1s, "h2": h2s, "dz1": [], "dz2": [], "dz3": []}
    with torch.no_grad():
        for t, (pre, head) in enumerate(TRUNKS):
            (W1, _), (W2, _) = R._layers(P, pre)
            i1, i2 = sorted({int(n.split(".")[1]) for n in P if n.startswith(pre + ".")})
            g_head = g_mean if t == 0 else g_value[:, None]
            At = g_head.shape[1]
            dz3 = torch.zeros(g_head.shape[0], HEAD_TILE, dtype=g_head.dtype, device=g_head.device)
            dz3[:, :At] = rnd(g_head)
            h1, h2 = h1s[t], h2s[t]
            p2 = (dz3[:, :At] @ rnd(P[head + ".weight"].detach())) * (1 - h2 * h2)
            dz2 = rnd(p2)
            p1 = (dz2 @ rnd(W2.detach())) * (1 - h1 * h1)
            dz1 = rnd(p1)
            grads[head + ".weight"] = dz3[:, :At].t() @ h2
            grads[head + ".bias"] = dz3[:, :At].sum(0)
            grads["%s.%d.weight" % (pre, i2)] = dz2.t() @ h1
            grads["%s.%d.weight" % (pre, i1)] = dz1.t() @ xb
            grads["%s.%d.bias" % (pre, i2)] = (dz2 if route == "wgrad" else p2).sum(0)
            grads["%s.%d.bias" % (pre, i1)] = (dz1 if route == "wgrad" else p1).sum(0)
            inter["dz1"].append(dz1)
            inter["dz2"].append(dz2)
            inter["dz3"].append(dz3)
    return total.detach(), out8, {n: grads[n] for n in P}, inter


# ------------------------------------------------------------------------------------------------ inputs of the kernel tests
BAND = 1e-2                  # no row's log ratio lies this close to log(1 - clip) or log(1 + clip)


def make_batch(P, D, A, B, seed, clip_range=0.2):
    """A minibatch whose ratios straddle the clip range (as _minibatch of test_learner_g1_shapes.py): actions drawn from the
    policy, old_logp = logp + 0.15 N(0, 1), advantages 2 N(0, 1) + 0.3.  A row whose log ratio (of the mirrored chain, fp64)
    lies within BAND of log(1 - clip) or log(1 + clip) has its old_logp moved by 0.02 away from that boundary: a clip decision
    that differs between kernel and reference would change the gradient by a whole row's worth."""
    import math
    dev = P["log_std"].device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    with torch.no_grad():
        obs = rn(B, D) * 0.7
        mean, _ = R.heads(P, obs)
        act = (mean + P["log_std"].exp() * rn(B, A).double()).float()
        old_logp = (R.logp(act, mean, P["log_std"]) + 0.15 * rn(B).double()).float()
        adv = rn(B) * 2 + 0.3
        ret = rn(B)
        lr = log_ratio(P, (obs, act, adv, ret, old_logp))
        for edge in (math.log1p(-clip_range), math.log1p(clip_range)):
            near = (lr - edge).abs() < BAND
            old_logp = torch.where(near, (old_logp.double() - torch.where(lr >= edge, 0.02, -0.02)).float(), old_logp)
    return obs.contiguous(), act.contiguous(), adv, ret, old_logp.contiguous()


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def max_rel(got, ref):
    """Largest absolute difference over the reference's largest entry."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the shapes and their bounds
# (arch, D, A, B, normalize, ent_coef, folds): the smallest shapes that reach each branch of the kernel (test_ppo_wide_kernel_gpu.py)
SHAPES = {
    "256x128-d1-a1-b64": ((256, 128), 1, 1, 64, False, 0.0, False),
    "256x128-d85-a23-b1024": ((256, 128), 85, 23, 1024, True, 0.01, True),
    "512x384-d112-a32-b192": ((512, 384), 112, 32, 192, True, 0.0, True),
    "768x256-d98-a23-b128": ((768, 256), 98, 23, 128, False, 0.01, True),
    "1024x512-d67-a28-b256": ((1024, 512), 67, 28, 256, True, 0.01, True),
    "256x128-d17-a2-b8256": ((256, 128), 17, 2, 8256, True, 0.0, True),
}
SEEDS = (11, 12, 13)         # input seeds of the measurement; the tests run the first
BOUNDS = {
    "256x128-d1-a1-b64": {
        "l2": {
            "log_std": 2.1e-05, "pi.0.weight": 0.00012, "pi.0.bias": 0.0018, "pi.2.weight": 0.00058, "pi.2.bias": 0.0019,
            "vf.0.weight": 0.00068, "vf.0.bias": 0.00075, "vf.2.weight": 0.00068, "vf.2.bias": 0.00014,
            "action_net.weight": 0.0026, "action_net.bias": 2.1e-05, "value_net.weight": 0.0013, "value_net.bias": 6.2e-05},
        "max": {
            "log_std": 2.1e-05, "pi.0.weight": 0.00042, "pi.0.bias": 0.0015, "pi.2.weight": 0.0032, "pi.2.bias": 0.0041,
            "vf.0.weight": 0.0017, "vf.0.bias": 0.00087, "vf.2.weight": 0.0021, "vf.2.bias": 0.00052,
            "action_net.weight": 0.0075, "action_net.bias": 2.1e-05, "value_net.weight": 0.0036, "value_net.bias": 6.2e-05},
        "stage": {
            "h1.0": 0.0005, "h1.1": 0.00044, "h2.0": 0.002, "h2.1": 0.0027, "dz3.0": 0.00049, "dz3.1": 0.00049,
            "dz2.0": 6.1e-05, "dz2.1": 0.0017, "dz1.0": 0.00024, "dz1.1": 0.0037},
    },
    "256x128-d85-a23-b1024": {
        "l2": {
            "log_std": 3.8e-05, "pi.0.weight": 0.0026, "pi.0.bias": 0.002, "pi.2.weight": 0.0018, "pi.2.bias": 0.0014,
            "vf.0.weight": 0.0012, "vf.0.bias": 0.00025, "vf.2.weight": 0.0009, "vf.2.bias": 0.00023,
            "action_net.weight": 0.0012, "action_net.bias": 0.0013, "value_net.weight": 0.00077, "value_net.bias": 2.4e-05},
        "max": {
            "log_std": 4.4e-05, "pi.0.weight": 0.0057, "pi.0.bias": 0.0017, "pi.2.weight": 0.0029, "pi.2.bias": 0.0016,
            "vf.0.weight": 0.00089, "vf.0.bias": 0.00021, "vf.2.weight": 0.0011, "vf.2.bias": 0.00084,
            "action_net.weight": 0.0044, "action_net.bias": 0.0031, "value_net.weight": 0.0011, "value_net.bias": 2.4e-05},
        "stage": {
            "h1.0": 0.00028, "h1.1": 0.00027, "h2.0": 0.00088, "h2.1": 0.00082, "dz3.0": 0.0011, "dz3.1": 0.0016,
            "dz2.0": 0.0018, "dz2.1": 0.0019, "dz1.0": 0.0025, "dz1.1": 0.0023},
    },
    "512x384-d112-a32-b192": {
        "l2": {
            "log_std": 3.5e-05, "pi.0.weight": 0.0024, "pi.0.bias": 0.0023, "pi.2.weight": 0.0012, "pi.2.bias": 0.0012,
            "vf.0.weight": 0.0023, "vf.0.bias": 0.00067, "vf.2.weight": 0.00092, "vf.2.bias": 0.00035,
            "action_net.weight": 0.00096, "action_net.bias": 0.00075, "value_net.weight": 0.0012, "value_net.bias": 0.00028},
        "max": {
            "log_std": 4.1e-05, "pi.0.weight": 0.015, "pi.0.bias": 0.0085, "pi.2.weight": 0.0029, "pi.2.bias": 0.0027,
            "vf.0.weight": 0.0042, "vf.0.bias": 0.0016, "vf.2.weight": 0.0013, "vf.2.bias": 0.00057,
            "action_net.weight": 0.0048, "action_net.bias": 0.0014, "value_net.weight": 0.0026, "value_net.bias": 0.00028},
        "stage": {
            "h1.0": 0.00035, "h1.1": 0.00034, "h2.0": 0.0013, "h2.1": 0.0013, "dz3.0": 0.00078, "dz3.1": 0.00098,
            "dz2.0": 0.0013, "dz2.1": 0.0012, "dz1.0": 0.0024, "dz1.1": 0.0027},
    },
    "768x256-d98-a23-b128": {
        "l2": {
            "log_std": 4.3e-05, "pi.0.weight": 0.0032, "pi.0.bias": 0.003, "pi.2.weight": 0.0017, "pi.2.bias": 0.0016,
            "vf.0.weight": 0.0015, "vf.0.bias": 0.0026, "vf.2.weight": 0.00059, "vf.2.bias": 0.00093,
            "action_net.weight": 0.0018, "action_net.bias": 0.00065, "value_net.weight": 0.0012, "value_net.bias": 2.1e-05},
        "max": {
            "log_std": 5.7e-05, "pi.0.weight": 0.0082, "pi.0.bias": 0.0051, "pi.2.weight": 0.0064, "pi.2.bias": 0.0029,
            "vf.0.weight": 0.0036, "vf.0.bias": 0.0041, "vf.2.weight": 0.0024, "vf.2.bias": 0.0034,
            "action_net.weight": 0.0064, "action_net.bias": 0.0019, "value_net.weight": 0.004, "value_net.bias": 2.1e-05},
        "stage": {
            "h1.0": 0.00043, "h1.1": 0.00029, "h2.0": 0.0016, "h2.1": 0.0016, "dz3.0": 0.0007, "dz3.1": 0.00035,
            "dz2.0": 0.0017, "dz2.1": 0.00055, "dz1.0": 0.0031, "dz1.1": 0.0015},
    },
    "1024x512-d67-a28-b256": {
        "l2": {
            "log_std": 7.3e-05, "pi.0.weight": 0.0059, "pi.0.bias": 0.0055, "pi.2.weight": 0.0043, "pi.2.bias": 0.004,
            "vf.0.weight": 0.0029, "vf.0.bias": 0.0018, "vf.2.weight": 0.0014, "vf.2.bias": 0.0008,
            "action_net.weight": 0.0031, "action_net.bias": 0.0024, "value_net.weight": 0.0016, "value_net.bias": 0.00061},
        "max": {
            "log_std": 0.00014, "pi.0.weight": 0.02, "pi.0.bias": 0.011, "pi.2.weight": 0.013, "pi.2.bias": 0.0088,
            "vf.0.weight": 0.0064, "vf.0.bias": 0.0035, "vf.2.weight": 0.0025, "vf.2.bias": 0.0027,
            "action_net.weight": 0.0082, "action_net.bias": 0.0037, "value_net.weight": 0.0026, "value_net.bias": 0.00061},
        "stage": {
            "h1.0": 0.00032, "h1.1": 0.00029, "h2.0": 0.0017, "h2.1": 0.0014, "dz3.0": 0.0027, "dz3.1": 0.0012,
            "dz2.0": 0.0045, "dz2.1": 0.0015, "dz1.0": 0.0062, "dz1.1": 0.0029},
    },
    "256x128-d17-a2-b8256": {
        "l2": {
            "log_std": 2.1e-05, "pi.0.weight": 0.0011, "pi.0.bias": 0.0018, "pi.2.weight": 0.00061, "pi.2.bias": 0.00095,
            "vf.0.weight": 0.00038, "vf.0.bias": 0.00031, "vf.2.weight": 0.00031, "vf.2.bias": 0.00024,
            "action_net.weight": 0.0014, "action_net.bias": 0.00044, "value_net.weight": 0.00029, "value_net.bias": 0.00026},
        "max": {
            "log_std": 2.1e-05, "pi.0.weight": 0.0027, "pi.0.bias": 0.0018, "pi.2.weight": 0.0015, "pi.2.bias": 0.0018,
            "vf.0.weight": 0.00039, "vf.0.bias": 0.00031, "vf.2.weight": 0.00039, "vf.2.bias": 0.00032,
            "action_net.weight": 0.0031, "action_net.bias": 0.00047, "value_net.weight": 0.00029, "value_net.bias": 0.00026},
        "stage": {
            "h1.0": 0.00029, "h1.1": 0.00029, "h2.0": 0.0011, "h2.1": 0.00098, "dz3.0": 8.9e-05, "dz3.1": 0.0014,
            "dz2.0": 0.00039, "dz2.1": 0.0017, "dz1.0": 0.0011, "dz1.1": 0.0021},
    },
}
