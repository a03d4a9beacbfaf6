"""CPU tests of the split-bf16 ("bf16x3") learner's reference (tests/ppo_wide3_ref64.py), of what its bounds catch, and of the host
side of the new entry points (dm_ppo_wide3_supported / _packed_elems are host functions; PPO's option check needs no GPU)."""
import functools

import pytest
import torch
import torch.nn as nn

import ppo_ref64 as R
import ppo_wide_ref64 as W
import ppo_wide3_ref64 as W3

KEYS = list(W.SHAPES)
DEFECTS = ("lo h1", "cross l2", "cross dw2", "tanh hi")


def _policy(arch, D, A, seed=13):
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=arch)
    with torch.no_grad():
        pol.log_std.add_(0.1 * torch.randn(A))
        for m in pol.modules():
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
    return pol


@functools.lru_cache(maxsize=None)
def _case(key):
    """(P, batch, keyword arguments of the loss, mirrored chain's result) of a shape of the GPU tests, on the CPU, first seed."""
    arch, D, A, B, normalize, ent, _ = W.SHAPES[key]
    P = R.params64(_policy(arch, D, A))
    batch = W3.make_batch(P, D, A, B, W.SEEDS[0])
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=ent, normalize=normalize)
    return P, batch, kw, W3.wide3_chain(P, batch, **kw)


# ------------------------------------------------------------------------------------------------ the split
def test_split_reproduces_an_fp32_value_to_2_pow_minus_16():
    """hi + lo is within 2^-16 relative of the fp32 value (measured: 2^-17), the sum is exact in fp32, lo is at most half an ulp
    of hi, and zero, powers of two and bf16 values split into (x, 0)."""
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(100000, generator=g) * torch.logspace(-6, 6, 100000), torch.tensor([0.0, 1.0, -2.0, 0.5, 1.0078125, 3.0e38, 1e-30])])
    hi, lo = W3.round_split(x)
    assert hi.dtype == torch.float32 and torch.equal(hi, hi.to(torch.bfloat16).float()) and torch.equal(lo, lo.to(torch.bfloat16).float())
    assert torch.equal((hi + lo).double(), hi.double() + lo.double())                 # exact in fp32
    rel = ((hi.double() + lo.double() - x.double()).abs() / x.double().abs().clamp_min(1e-300))
    assert float(rel.max()) <= 2.0 ** -16, float(rel.max())
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -8).all())
    exact = x.to(torch.bfloat16).float() == x
    assert bool((lo[exact] == 0).all()) and torch.equal(hi[exact], x[exact])
    h64, l64 = W3.round_split(x.double())
    assert h64.dtype == torch.float64 and torch.equal(h64, hi.double()) and torch.equal(l64, lo.double())


def test_three_term_product_is_the_product_without_lo_lo():
    """mm3 = a @ b - a_lo @ b_lo, in the closed form and as the three sums the kernel forms; a dropped cross term is that term."""
    g = torch.Generator().manual_seed(4)
    a, b = W3.round_split(torch.randn(24, 48, generator=g).double()), W3.round_split(torch.randn(48, 40, generator=g).double())
    full = W3.val(a) @ W3.val(b)
    assert torch.allclose(W3.mm3(a, b), full - a[1] @ b[1], rtol=0, atol=1e-15)
    assert torch.allclose(W3.mm3(a, b, three_sums=True), W3.mm3(a, b), rtol=0, atol=1e-14)
    assert torch.allclose(W3.mm3(a, b, drop="lo.hi"), W3.mm3(a, b) - a[1] @ b[0], rtol=0, atol=1e-14)
    assert torch.allclose(W3.mm3(a, b, drop="hi.lo"), W3.mm3(a, b) - a[0] @ b[1], rtol=0, atol=1e-14)
    assert float((W3.mm3(a, b) - full).abs().max()) <= 48 * 2.0 ** -16 * float(full.abs().max())


def test_unrounded_chain_equals_autograd():
    """With no split the chain's loss and every gradient equal ppo_ref64.grads (fp64 autograd) to 1e-12: pins the hand-written
    backward of this module, both bias routes."""
    D, A, B = 19, 5, 96
    P = R.params64(_policy((48, 40), D, A, seed=5))
    batch = W.make_batch(P, D, A, B, 5)
    kw = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, normalize=True)
    l0, o0, g0 = R.grads(P, *batch, **kw)
    for route in ("chain", "wgrad"):
        l1, o1, g1, _ = W3.unrounded_chain(P, batch, bias_route=route, **kw)
        assert abs(float(l1 - l0)) <= 1e-12 and float((o1 - o0).abs().max()) <= 1e-12
        for n in g0:
            assert W.rel_l2(g1[n], g0[n]) <= 1e-12 and W.max_rel(g1[n], g0[n]) <= 1e-12, n


# ------------------------------------------------------------------------------------------------ accuracy of the number format
@pytest.mark.parametrize("key", KEYS)
def test_mirrored_chain_is_within_1e_4_of_the_unrounded_chain(key):
    """Every gradient tensor of the mirrored fp64 chain within 1e-4 relative L2 and 1e-4 of the largest entry of the unrounded
    fp64 chain (the bound the GPU test holds the kernel to; measured on the six shapes: <= 1.5e-5 and <= 2.3e-5)."""
    P, batch, kw, (_, _, g, _) = _case(key)
    gu = W3.unrounded_chain(P, batch, **kw)[2]
    worst = (max(W.rel_l2(g[n], gu[n]) for n in g), max(W.max_rel(g[n], gu[n]) for n in g))
    print("%-24s mirrored vs unrounded: rel L2 %.3g  max %.3g" % (key, *worst))
    for n in g:
        assert float(gu[n].abs().max()) > 0, n
        assert W.rel_l2(g[n], gu[n]) <= W3.UNROUNDED_BOUND and W.max_rel(g[n], gu[n]) <= W3.UNROUNDED_BOUND, (key, n)


@pytest.mark.parametrize("key", KEYS)
def test_fp32_evaluation_is_inside_the_bounds_and_the_differing_cap(key):
    """The mirrored chain evaluated as the kernel's formats evaluate it (ppo_wide3_ref64.evaluate32) against the same chain in
    fp64: every quantity within a tenth of its bound (the rule BOUNDS were set by, first of the three seeds), and the hi plane of
    every stage differs in at most 1 % of its elements: well inside the 5 % cap the GPU test puts on the kernel."""
    P, batch, kw, (_, _, g, it) = _case(key)
    _, _, g32, it32 = W3.evaluate32(P, batch, **kw)
    q = W3.measure(g32, it32, g, it)
    bd = W3.BOUNDS[key]
    for n in g:
        assert 10 * q["l2"][n] <= bd["l2"][n] * 1.0001 and 10 * q["max"][n] <= bd["max"][n] * 1.0001, (key, n, q["l2"][n], q["max"][n])
    for sk, v in q["stage"].items():
        assert 10 * v <= bd["stage"][sk] * 1.0001, (key, sk, v)
        assert q["differing"][sk] <= 0.01, (key, sk, q["differing"][sk])


# ------------------------------------------------------------------------------------------------ what the bounds catch
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("defect", DEFECTS)
def test_defect_models_exceed_the_bounds(defect, key):
    """Each defect model of ppo_wide3_ref64.wide3_chain moves at least one gradient tensor or stage of the mirrored chain beyond 3 x
    its bound in BOUNDS: the lo plane of one operand (h1) dropped, one cross term dropped (in layer 2; in dW2), tanh' taken from
    the hi plane alone.  Printed with -s: the largest distance / bound."""
    P, batch, kw, (_, _, g, it) = _case(key)
    _, _, gd, itd = W3.wide3_chain(P, batch, defect=defect, **kw)
    q = W3.measure(gd, itd, g, it)
    bd = W3.BOUNDS[key]
    factor = max([q["l2"][n] / bd["l2"][n] for n in g] + [q["max"][n] / bd["max"][n] for n in g] + [v / bd["stage"][sk] for sk, v in q["stage"].items()])
    print("%-24s %-10s largest distance / bound %8.1f" % (key, defect, factor))
    assert factor >= 3.0, (key, defect, factor)


# ------------------------------------------------------------------------------------------------ host side of the entry points
def _lib():
    from deepmimic_mujoco_amd import _lib as L
    return L.load_library()


def test_wide3_supported_truth_table_and_packed_elems():
    """dm_ppo_wide3_supported: every shape of SHAPES, [1024,512] with D = 112 and every shape dm_ppo_wide_supported takes on a grid;
    the five refusals of the bf16 kernel's test (B = 96, H1 = 384, H2 = 192, D = 113, A = 33) and the edges around them.
    dm_ppo_wide3_packed_elems = both planes = 2 x (H1 Dp + 2 H1 H2 + 64 H2)."""
    L = _lib()
    for arch, D, A, B, *_ in W.SHAPES.values():
        assert L.dm_ppo_wide3_supported(B, D, arch[0], arch[1], A) == 1
        assert L.dm_ppo_wide3_packed_elems(D, *arch) == 2 * (arch[0] * W.dp(D) + 2 * arch[0] * arch[1] + 64 * arch[1]) == 2 * L.dm_ppo_wide_packed_elems(D, *arch)
    assert L.dm_ppo_wide3_supported(4096, 112, 1024, 512, 32) == 1 and L.dm_ppo_wide3_supported(64, 1, 256, 128, 1) == 1
    base = dict(B=1024, D=85, H1=256, H2=128, A=23)
    for field, value in (("B", 96), ("H1", 384), ("H2", 192), ("D", 113), ("A", 33), ("B", 0), ("B", 32), ("D", 0), ("A", 0), ("H1", 1280), ("H2", 640),
                         ("H1", 0), ("H2", 0)):
        d = dict(base, **{field: value})
        assert L.dm_ppo_wide3_supported(d["B"], d["D"], d["H1"], d["H2"], d["A"]) == 0, (field, value)
    for B in (64, 96, 128, 4096):
        for D in (1, 16, 67, 112, 113):
            for H1 in (256, 384, 512, 768, 1024, 1280):
                for H2 in (128, 192, 256, 384, 512, 640):
                    for A in (1, 28, 32, 33):
                        if L.dm_ppo_wide_supported(B, D, H1, H2, A):
                            assert L.dm_ppo_wide3_supported(B, D, H1, H2, A) == 1, (B, D, H1, H2, A)


def test_wide3_grad_refuses_a_null_step_without_a_device():
    assert _lib().dm_ppo_wide3_grad(None, None) == -22


def test_ppo_bf16x3_on_the_cpu_raises():
    """PPO(mlp_dtype="bf16x3") needs the flat Adam path, as mlp_dtype=torch.bfloat16 does: a ValueError on the CPU."""
    from deepmimic_mujoco_amd.ppo import PPO
    for dt in ("bf16x3", torch.bfloat16):
        with pytest.raises(ValueError, match="flat Adam"):
            PPO(None, net_arch=(1024, 512), batch_size=256, device=torch.device("cpu"), mlp_dtype=dt)


def test_ppo_mlp_dtype_is_validated_and_the_library_paths_are_named():
    """Anything but torch.float32, torch.bfloat16 or "bf16x3" is a ValueError (a misspelt "bf16x2" must not silently take the fp32
    library path); a learner without the flat Adam path reports "library_fp32", and routes every minibatch to the library."""
    from deepmimic_mujoco_amd.ppo import PPO
    for bad in ("bf16x2", "bfloat16", torch.float16, None):
        with pytest.raises(ValueError, match="mlp_dtype"):
            PPO(None, net_arch=(64, 64), batch_size=64, device=torch.device("cpu"), mlp_dtype=bad)
    for arch in ((1024, 512), (256, 128)):
        ppo = PPO(None, net_arch=arch, batch_size=256, device=torch.device("cpu"))
        assert ppo.learner_path() == "library_fp32"
        assert ppo._grad_route(256, on_gpu=False) == "library" and ppo._grad_route(128, on_gpu=False) == "library"


# ------------------------------------------------------------------------------------------------ the rule behind BOUNDS
def test_committed_bounds_follow_the_rule_on_the_smallest_shape():
    """ppo_wide3_ref64.bounds_for regenerates BOUNDS of the smallest shape from the three seeds (10 x the fp32 self-distance, the
    floors, two digits rounded up): every committed value within one step of the second digit (a factor 1.1) of the regenerated one.
    Not exact equality: the fp32 matmuls of evaluate32 sum in the order the CPU's BLAS chooses, which may move a value across a
    rounding step.  An inflated or stale bound fails."""
    key = "256x128-d1-a1-b64"
    arch, D, A, *_ = W.SHAPES[key]
    gen = W3.bounds_for(R.params64(_policy(arch, D, A)), key)
    for q in ("l2", "max", "stage"):
        assert set(gen[q]) == set(W3.BOUNDS[key][q])
        for n, v in gen[q].items():
            assert v / 1.1001 <= W3.BOUNDS[key][q][n] <= v * 1.1001, (q, n, v, W3.BOUNDS[key][q][n])
    assert W3.round_up2(1.01e-5) == 1.1e-5 and W3.round_up2(2e-5) == 2e-5 and W3.round_up2(9.91e-4) == 1e-3
