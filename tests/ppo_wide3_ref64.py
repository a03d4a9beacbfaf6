"""fp64 reference of ``dm_ppo_wide3_grad`` (csrc/dm_ppo_wide3.hip, the "bf16x3" learner) that splits where the kernel splits
(test helper, not a conftest).  Plain torch, ``ppo_ref64`` and ``ppo_wide_ref64`` only: nothing of the product is imported.

The kernel carries every operand of a product as two bf16 planes, ``hi = rne_bf16(x)``, ``lo = rne_bf16(x - hi)`` (``round_split``),
and forms ``a b`` as ``a_lo b_hi + a_hi b_lo + a_hi b_hi`` with fp32 accumulation: ``a b`` without ``a_lo b_lo`` (``mm3``).  Its
rounding points are those of the bf16 kernel (docstring of ppo_wide_ref64.py), each a split: obs, every weight, h1, h2, dZ3, dZ2,
dZ1.  Everything that is not a product sees ``hi + lo``: tanh' = 1 - (hi + lo)^2, the column sums.

Bias routes (``ppo_wide_ref64.BIAS_WGRAD_H1`` = 512, as the bf16 kernel): H1 >= 512 ("wgrad"): all three bias gradients are column
sums of the SPLIT dZ (both planes times a fragment of ones); H1 < 512 ("chain"): gb3 sums the split dZ3, gb2 / gb1 the unrounded
fp32 products.

BOUNDS at the end of the file, per shape and quantity, by the rule of ppo_wide_ref64.py: 10 x the distance of this chain evaluated
in fp32 (``evaluate32``: fp32 parameters, the kernel's tanh 1 - 2 / (1 + exp(2 x)), the three terms of a product summed in fp32)
from the same chain in fp64, on the CPU, worst of the input seeds 11, 12, 13.  Floors: 2e-5 for a gradient; for a stage one element
off by one ulp of its lo plane, 2^-16 / sqrt(elements).  An MI355X sweep of the kernel over the three seeds confirmed every
bound (smallest margin 4.3 x).  The device-rule set, 4 x the kernel's worst measured distance over the three seeds, is recorded in
DESIGN section 15 beside this one and is not applied.
``bounds_for`` generates this set.
"""
import math

import torch

import ppo_ref64 as R
import ppo_wide_ref64 as W

TRUNKS, BIAS_WGRAD_H1, HEAD_TILE, SHAPES, SEEDS = W.TRUNKS, W.BIAS_WGRAD_H1, W.HEAD_TILE, W.SHAPES, W.SEEDS
UNROUNDED_BOUND = 1e-4       # every gradient of the kernel against the UNROUNDED fp64 chain, relative L2 and max over the largest entry
GRAD_FLOOR = 2e-5


def round_split(x):
    """(hi, lo) in x's dtype: hi = bf16(fp32(x)), lo = bf16(fp32(x) - hi); hi + lo is exact in fp32."""
    f = x.float()
    hi = f.to(torch.bfloat16).float()
    lo = (f - hi).to(torch.bfloat16).float()
    return hi.to(x.dtype), lo.to(x.dtype)


def val(s):
    return s[0] + s[1]


def tr(s):
    return s[0].t(), s[1].t()


def mm3(a, b, three_sums=False, drop=None):
    """a @ b of two split operands without a_lo @ b_lo.  three_sums: the kernel's order lo.hi + hi.lo + hi.hi, each term a matmul
    of the working dtype (the fp32 evaluation); drop: a defect model, "lo.hi" or "hi.lo" leaves that cross term out."""
    (ah, al), (bh, bl) = a, b
    if three_sums or drop:
        out = ah @ bh
        if drop != "hi.lo":
            out = ah @ bl + out
        if drop != "lo.hi":
            out = al @ bh + out
        return out
    return (ah + al) @ (bh + bl) - al @ bl


def fast_tanh(x):
    """The kernel's activation (ppo_fast_tanh) in x's dtype."""
    return 1 - 2 / (1 + torch.exp(2 * x))


def stage_floor(numel):
    return 2.0 ** -16 / math.sqrt(numel)


def packed_reference(P_trunk, D, H1, H2, A_t):
    """(hi blocks, lo blocks): the five blocks of one trunk's packed weights (ppo_wide_ref64.packed_reference) as bf16 matrices,
    one list per plane."""
    W1, W2, W3 = (w.detach().float() for w in P_trunk)
    w1 = torch.zeros(H1, W.dp(D), device=W1.device)
    w1[:, :D] = W1
    w3 = torch.zeros(HEAD_TILE, H2, device=W1.device)
    w3[:A_t] = W3
    planes = ([], [])
    for m in (w1, W2, W2.t(), w3, w3.t()):
        for p, x in zip(planes, round_split(m.contiguous())):
            p.append(x.to(torch.bfloat16))
    return planes


def _forward(P, obs, split, tanh, mm):
    d = P["log_std"].dtype
    xb = split(obs.to(d))
    h1s, h2s, outs = [], [], []
    for pre, head in TRUNKS:
        (W1, b1), (W2, b2) = R._layers(P, pre)
        h1 = split(tanh(mm(xb, tr(split(W1.detach())), "l1") + b1.detach()))
        h2 = split(tanh(mm(h1, tr(split(W2.detach())), "l2") + b2.detach()))
        outs.append(mm(h2, tr(split(P[head + ".weight"].detach())), "l3") + P[head + ".bias"].detach())
        h1s.append(h1)
        h2s.append(h2)
    return xb, h1s, h2s, outs


def wide3_chain(P, batch, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True, bias_route=None, tanh=torch.tanh, three_sums=False,
                defect=None, split=round_split):
    """One minibatch of the bf16x3 learner with the kernel's split points, in P's dtype.  Same interface and structure as
    ppo_wide_ref64.wide_chain; intermediates hold (hi, lo) pairs: {"xb", "h1": [t], "h2": [t], "dz1": [t], "dz2": [t], "dz3": [t]}.

    split = lambda x: (x, 0 x) gives the UNROUNDED chain.  defect (models for tests/test_ppo_wide3_ref64.py):
      "lo h1"     the lo plane of h1 dropped where layer 2 and dW2 multiply it
      "cross l2"  the cross term h1_lo W2_hi dropped from layer 2's product
      "cross dw2" the cross term dZ2_hi h1_lo dropped from dW2
      "tanh hi"   tanh' of both layers from the hi plane alone"""
    def mm(a, b, where):
        if defect == "lo h1" and where in ("l2", "dw2"):
            if where == "l2":
                a = (a[0], torch.zeros_like(a[1]))
            else:
                b = (b[0], torch.zeros_like(b[1]))
        drop = "lo.hi" if (defect == "cross l2" and where == "l2") else "hi.lo" if (defect == "cross dw2" and where == "dw2") else None
        return mm3(a, b, three_sums, drop)
    tv = (lambda s: s[0]) if defect == "tanh hi" else val
    obs, act, adv, ret, old_logp = batch
    with torch.no_grad():
        xb, h1s, h2s, outs = _forward(P, obs, split, tanh, mm)
    mean = outs[0].clone().requires_grad_(True)
    value = outs[1].squeeze(-1).clone().requires_grad_(True)
    ls = P["log_std"].detach().clone().requires_grad_(True)
    total, out8 = R.head_loss(mean, ls, value, act, adv, ret, old_logp, clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef,
                              normalize=normalize)
    g_mean, g_value, g_ls = torch.autograd.grad(total, [mean, value, ls])
    H1 = h1s[0][0].shape[1]
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
            z = torch.zeros(g_head.shape[0], HEAD_TILE, dtype=g_head.dtype, device=g_head.device)
            z[:, :At] = g_head
            dz3 = split(z)
            live3 = (dz3[0][:, :At], dz3[1][:, :At])
            h1, h2 = h1s[t], h2s[t]
            p2 = mm(live3, split(P[head + ".weight"].detach()), "d2") * (1 - tv(h2) * tv(h2))
            dz2 = split(p2)
            p1 = mm(dz2, split(W2.detach()), "d1") * (1 - tv(h1) * tv(h1))
            dz1 = split(p1)
            grads[head + ".weight"] = mm(tr(live3), h2, "dw3")
            grads[head + ".bias"] = val(live3).sum(0)
            grads["%s.%d.weight" % (pre, i2)] = mm(tr(dz2), h1, "dw2")
            grads["%s.%d.weight" % (pre, i1)] = mm(tr(dz1), xb, "dw1")
            grads["%s.%d.bias" % (pre, i2)] = (val(dz2) if route == "wgrad" else p2).sum(0)
            grads["%s.%d.bias" % (pre, i1)] = (val(dz1) if route == "wgrad" else p1).sum(0)
            inter["dz1"].append(dz1)
            inter["dz2"].append(dz2)
            inter["dz3"].append(dz3)
    return total.detach(), out8, {n: grads[n] for n in P}, inter


def unsplit(x):
    return x, torch.zeros_like(x)


def unrounded_chain(P, batch, **kw):
    """The same chain with no rounding anywhere (fp64): what the learner would compute in exact arithmetic."""
    return wide3_chain(P, batch, split=unsplit, **kw)


def evaluate32(P, batch, **kw):
    """The mirrored chain as the kernel's number formats evaluate it: fp32 parameters and inputs, the kernel's tanh formula, the
    three terms of every product summed in fp32."""
    P32 = {n: p.detach().float().requires_grad_(True) for n, p in P.items()}
    return wide3_chain(P32, batch, tanh=fast_tanh, three_sums=True, **kw)


def log_ratio(P, batch):
    obs, act, _, _, old_logp = batch
    with torch.no_grad():
        _, _, _, outs = _forward(P, obs, round_split, torch.tanh, lambda a, b, w: mm3(a, b))
        return R.logp(act, outs[0], P["log_std"].detach()) - old_logp.to(outs[0])


def make_batch(P, D, A, B, seed, clip_range=0.2):
    """ppo_wide_ref64.make_batch with the exclusion band (ppo_wide_ref64.BAND) taken on THIS chain's log ratio: the bf16 chain's
    log ratio is up to ~1e-2 away from it, so its band would not keep this chain's rows off the clip boundaries."""
    obs, act, adv, ret, old_logp = W.make_batch(P, D, A, B, seed, clip_range)
    with torch.no_grad():
        for _ in range(4):
            lr = log_ratio(P, (obs, act, adv, ret, old_logp))
            moved = False
            for edge in (math.log1p(-clip_range), math.log1p(clip_range)):
                near = (lr - edge).abs() < W.BAND
                if bool(near.any()):
                    moved = True
                    old_logp = torch.where(near, (old_logp.double() - torch.where(lr >= edge, 0.02, -0.02)).float(), old_logp)
            if not moved:
                break
    return obs, act, adv, ret, old_logp.contiguous()


def measure(got_grads, got_inter, ref_grads, ref_inter):
    """{"l2", "max": per gradient; "stage": relative L2 of hi + lo per stage and trunk; "differing": fraction of hi-plane elements
    that differ} of one evaluation against another."""
    q = {"l2": {}, "max": {}, "stage": {}, "differing": {}}
    for n in ref_grads:
        q["l2"][n], q["max"][n] = W.rel_l2(got_grads[n], ref_grads[n]), W.max_rel(got_grads[n], ref_grads[n])
    for s in ("h1", "h2", "dz3", "dz2", "dz1"):
        for t in range(2):
            g, r = got_inter[s][t], ref_inter[s][t]
            q["stage"]["%s.%d" % (s, t)] = W.rel_l2(val(g), val(r))
            q["differing"]["%s.%d" % (s, t)] = float((g[0].double() != r[0].double()).double().mean())
    return q


# ------------------------------------------------------------------------------------------------ the bounds (module docstring)
def round_up2(x):
    """x rounded UP to two significant digits."""
    e = math.floor(math.log10(x))
    return float("%.2g" % (math.ceil(x / 10 ** e * 10 - 1e-9) / 10 * 10 ** e))


def bounds_for(P, key, seeds=SEEDS):
    """BOUNDS[key] by the rule of the module docstring, for the fp64 parameters P of a policy of SHAPES[key]'s sizes: 10 x the worst
    over `seeds` of evaluate32 against wide3_chain, floored, rounded up to two digits."""
    (H1, H2), D, A, B, normalize, ent, _ = SHAPES[key]
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=ent, normalize=normalize)
    worst = None
    for seed in seeds:
        batch = make_batch(P, D, A, B, seed)
        _, _, g, it = wide3_chain(P, batch, **kw)
        _, _, g32, it32 = evaluate32(P, batch, **kw)
        q = measure(g32, it32, g, it)
        worst = q if worst is None else {k: {n: max(worst[k][n], q[k][n]) for n in q[k]} for k in q}
    numel = {"h1": H1 * B, "dz1": H1 * B, "h2": H2 * B, "dz2": H2 * B}
    out = {"l2": {n: round_up2(max(10 * v, GRAD_FLOOR)) for n, v in worst["l2"].items()},
           "max": {n: round_up2(max(10 * v, GRAD_FLOOR)) for n, v in worst["max"].items()}, "stage": {}}
    for sk, v in worst["stage"].items():
        s, t = sk.split(".")
        out["stage"][sk] = round_up2(max(10 * v, stage_floor(numel.get(s, (A if t == "0" else 1) * B))))
    return out


BOUNDS = {
    "256x128-d1-a1-b64": {
        "l2": {
            "log_std": 2e-05, "pi.0.weight": 4.4e-05, "pi.0.bias": 0.00039, "pi.2.weight": 4.8e-05, "pi.2.bias": 0.00017,
            "vf.0.weight": 2e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight":
            6.8e-05, "action_net.bias": 0.00023, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "max": {
            "log_std": 2e-05, "pi.0.weight": 7.1e-05, "pi.0.bias": 0.00038, "pi.2.weight": 9.7e-05, "pi.2.bias": 0.00011,
            "vf.0.weight": 2.9e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2.3e-05, "vf.2.bias": 2e-05, "action_net.weight":
            0.00011, "action_net.bias": 0.00023, "value_net.weight": 2.2e-05, "value_net.bias": 2e-05},
        "stage": {
            "h1.0": 1.6e-05, "h1.1": 1.5e-05, "h2.0": 2.6e-05, "h2.1": 2.3e-05, "dz3.0": 4.8e-06, "dz3.1": 2.1e-05, "dz2.0":
            1.4e-05, "dz2.1": 2.5e-05, "dz1.0": 2.3e-05, "dz1.1": 2.9e-05},
    },
    "256x128-d85-a23-b1024": {
        "l2": {
            "log_std": 2.6e-05, "pi.0.weight": 5.8e-05, "pi.0.bias": 6.1e-05, "pi.2.weight": 4.9e-05, "pi.2.bias": 5e-05,
            "vf.0.weight": 2.1e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight":
            3.9e-05, "action_net.bias": 5e-05, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "max": {
            "log_std": 2e-05, "pi.0.weight": 6.4e-05, "pi.0.bias": 5.6e-05, "pi.2.weight": 5.2e-05, "pi.2.bias": 4.8e-05,
            "vf.0.weight": 2e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight":
            4.6e-05, "action_net.bias": 5.1e-05, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "stage": {
            "h1.0": 7.5e-06, "h1.1": 7.5e-06, "h2.0": 1.7e-05, "h2.1": 1.8e-05, "dz3.0": 3.5e-05, "dz3.1": 1.8e-05, "dz2.0":
            4.7e-05, "dz2.1": 2.6e-05, "dz1.0": 5.7e-05, "dz1.1": 3.5e-05},
    },
    "512x384-d112-a32-b192": {
        "l2": {
            "log_std": 3.6e-05, "pi.0.weight": 6e-05, "pi.0.bias": 6.1e-05, "pi.2.weight": 5.1e-05, "pi.2.bias": 5.4e-05,
            "vf.0.weight": 3.3e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2.1e-05, "vf.2.bias": 2e-05, "action_net.weight":
            4.3e-05, "action_net.bias": 4.1e-05, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "max": {
            "log_std": 5.9e-05, "pi.0.weight": 6.6e-05, "pi.0.bias": 6.4e-05, "pi.2.weight": 5.3e-05, "pi.2.bias": 5.6e-05,
            "vf.0.weight": 4.9e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight":
            5.1e-05, "action_net.bias": 5.2e-05, "value_net.weight": 2.1e-05, "value_net.bias": 2e-05},
        "stage": {
            "h1.0": 8.5e-06, "h1.1": 8.2e-06, "h2.0": 1.9e-05, "h2.1": 1.9e-05, "dz3.0": 3.9e-05, "dz3.1": 1.8e-05, "dz2.0":
            5.1e-05, "dz2.1": 2.6e-05, "dz1.0": 6e-05, "dz1.1": 3.6e-05},
    },
    "768x256-d98-a23-b128": {
        "l2": {
            "log_std": 3e-05, "pi.0.weight": 6.1e-05, "pi.0.bias": 7.7e-05, "pi.2.weight": 5.3e-05, "pi.2.bias": 6.1e-05,
            "vf.0.weight": 3.6e-05, "vf.0.bias": 5.1e-05, "vf.2.weight": 2.9e-05, "vf.2.bias": 3.5e-05, "action_net.weight":
            4.8e-05, "action_net.bias": 4.9e-05, "value_net.weight": 2.9e-05, "value_net.bias": 2e-05},
        "max": {
            "log_std": 4.1e-05, "pi.0.weight": 7.1e-05, "pi.0.bias": 8.6e-05, "pi.2.weight": 6.6e-05, "pi.2.bias": 6.6e-05,
            "vf.0.weight": 4.6e-05, "vf.0.bias": 0.00012, "vf.2.weight": 4.1e-05, "vf.2.bias": 7.3e-05, "action_net.weight":
            4.9e-05, "action_net.bias": 5.8e-05, "value_net.weight": 3.2e-05, "value_net.bias": 2e-05},
        "stage": {
            "h1.0": 8.7e-06, "h1.1": 9e-06, "h2.0": 2e-05, "h2.1": 2e-05, "dz3.0": 4.2e-05, "dz3.1": 1.9e-05, "dz2.0":
            5.2e-05, "dz2.1": 2.6e-05, "dz1.0": 6.1e-05, "dz1.1": 3.5e-05},
    },
    "1024x512-d67-a28-b256": {
        "l2": {
            "log_std": 3.3e-05, "pi.0.weight": 6e-05, "pi.0.bias": 5.8e-05, "pi.2.weight": 5e-05, "pi.2.bias": 4.9e-05,
            "vf.0.weight": 2.8e-05, "vf.0.bias": 4.2e-05, "vf.2.weight": 2.3e-05, "vf.2.bias": 3.2e-05, "action_net.weight":
            4.5e-05, "action_net.bias": 4.1e-05, "value_net.weight": 2.6e-05, "value_net.bias": 2.7e-05},
        "max": {
            "log_std": 3.3e-05, "pi.0.weight": 7.1e-05, "pi.0.bias": 7.3e-05, "pi.2.weight": 6.9e-05, "pi.2.bias": 5.8e-05,
            "vf.0.weight": 2.2e-05, "vf.0.bias": 5.7e-05, "vf.2.weight": 2.6e-05, "vf.2.bias": 3.8e-05, "action_net.weight":
            5.2e-05, "action_net.bias": 5.4e-05, "value_net.weight": 3.2e-05, "value_net.bias": 2.7e-05},
        "stage": {
            "h1.0": 1.1e-05, "h1.1": 9.8e-06, "h2.0": 2.2e-05, "h2.1": 2.1e-05, "dz3.0": 4.1e-05, "dz3.1": 1.8e-05, "dz2.0":
            5.1e-05, "dz2.1": 2.2e-05, "dz1.0": 6e-05, "dz1.1": 3.1e-05},
    },
    "256x128-d17-a2-b8256": {
        "l2": {
            "log_std": 2e-05, "pi.0.weight": 3e-05, "pi.0.bias": 8.5e-05, "pi.2.weight": 2.5e-05, "pi.2.bias": 7e-05,
            "vf.0.weight": 2e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight":
            2.9e-05, "action_net.bias": 7.4e-05, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "max": {
            "log_std": 2e-05, "pi.0.weight": 2.8e-05, "pi.0.bias": 9.1e-05, "pi.2.weight": 2.2e-05, "pi.2.bias": 7e-05,
            "vf.0.weight": 2e-05, "vf.0.bias": 2e-05, "vf.2.weight": 2e-05, "vf.2.bias": 2e-05, "action_net.weight": 3e-05,
            "action_net.bias": 7.6e-05, "value_net.weight": 2e-05, "value_net.bias": 2e-05},
        "stage": {
            "h1.0": 9.6e-06, "h1.1": 9.6e-06, "h2.0": 2.1e-05, "h2.1": 2.1e-05, "dz3.0": 1.4e-05, "dz3.1": 1.8e-05, "dz2.0":
            1.9e-05, "dz2.1": 2.3e-05, "dz1.0": 2.8e-05, "dz1.1": 3e-05},
    },
}
