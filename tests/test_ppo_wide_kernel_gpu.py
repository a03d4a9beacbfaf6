"""dm_ppo_wide_grad (csrc/dm_ppo_wide.hip) called directly through DmPpoWideStep, with buffers the test owns, against the fp64
reference that rounds where the kernel rounds (tests/ppo_wide_ref64.py).

Shapes (ppo_wide_ref64.SHAPES), the smallest that reach each branch; none is the workload's own size:

| arch       | D   | A  | B    | norm | ent  | folds | reaches                                                                              |
| (256,128)  | 1   | 1  | 64   | off  | 0    | none  | Dp = 16 with one k-step, the smallest head, 2 row tiles in plain order, only wave 3  |
|            |     |    |      |      |      |       | of a weight-gradient workgroup has rows, accumulate semantics, bias in the chain     |
| (256,128)  | 85  | 23 | 1024 | on   | 0.01 | all   | split-K 8 with atomics on dW2, split-K on the heads, XCD block order                 |
| (512,384)  | 112 | 32 | 192  | on   | 0    | all   | D = Dp, full action tile, 3 head k-steps per wave, 6 row tiles in plain order, an    |
|            |     |    |      |      |      |       | uneven wave split of 3 batch units, bias from the weight-gradient launch             |
| (768,256)  | 98  | 23 | 128  | off  | 0.01 | all   | three layer-1 tiles per wave (pa / pb / pa prefetch), 4 row tiles: smallest XCD order |
| (1024,512) | 67  | 28 | 256  | on   | 0.01 | all   | the product net, every wave busy in every stage, split-K 1 everywhere                |
| (256,128)  | 17  | 2  | 8256 | on   | 0    | all   | the B > 8192 statistics routine                                                      |

Every output and scratch array is a view at the front of a buffer filled with NaN (fp32) or 0x7FC0 (bf16) with a guard region
behind it.  Bounds: ppo_wide_ref64.BOUNDS, per shape and quantity.  They are UNMEASURED ON THE DEVICE (no MI355X run could be
had when they were set): 10 x the fp32-against-fp64 self-distance of the mirrored chain on the CPU, worst of the three input
seeds ppo_wide_ref64.SEEDS (worst self-distance over all shapes: gradients 5.9e-4 relative L2 and 1.9e-3 of the largest entry,
stages 6.1e-4, 1.6 % of a stage's elements differing; DESIGN.md section 14 tabulates them per shape).  Run with -s for the
"measured / bound / margin" lines of the kernel itself.
"""
import functools

import pytest
import torch

import ppo_wide_ref64 as W
from kernel_helpers import DEV, check_out8, guard_ok as _guard_ok, lib as _lib, note, stream as _stream
from wide_call import WideCall

pytestmark = pytest.mark.gpu

KEYS = list(W.SHAPES)
MAX_DIFFERING = 0.05     # at most this fraction of a stage's elements may differ at all from the reference's bf16 value
STAGES = ("h1", "h2", "dz3", "dz2", "dz1")

_note = functools.partial(note, width=46)
_check_out8 = functools.partial(check_out8, width=46)


class _Call(WideCall):
    """The buffers of one dm_ppo_wide_grad call and its DmPpoWideStep."""

    entry, packed_elems, supported, step_cls = "dm_ppo_wide_grad", "dm_ppo_wide_packed_elems", "dm_ppo_wide_supported", "DmPpoWideStep"
    planes, ref = 1, W

    def T(self, name, N):
        """A transposed scratch array [N][B], un-fragmented, as int16."""
        return W.unfrag(self.bf[name][1], N, self.dims[0])


class _Run:
    """One launch and the mirrored reference of the same minibatch."""

    def __init__(self, key, seed):
        c = self.c = _Call(key, seed)
        assert c.launch() == 0
        self.loss, self.ref8, self.gref, self.inter = W.wide_chain(c.P, c.batch, clip_range=c.clip, vf_coef=c.vf, ent_coef=c.ent,
                                                                   normalize=c.normalize)
        self.ratio64 = torch.exp(W.log_ratio(c.P, c.batch))

    def stage(self, s, t):
        """(kernel's array [N][B] as fp64, reference's [N][B]) of stage s, trunk t; dz3: the live head rows only."""
        c = self.c
        B, D, H1, H2, A = c.dims
        N = {"h1": H1, "dz1": H1, "h2": H2, "dz2": H2, "dz3": 32}[s]
        got = c.T("%sT%d" % (s, t), N).view(torch.bfloat16).double()
        ref = self.inter[s][t].t()
        if s == "dz3":
            live = A if t == 0 else 1
            got, ref = got[:live], ref[:live]
        return got, ref

    def quantities(self):
        """{"l2": {name: relative L2}, "max": {name: max-abs over the largest entry}, "stage": {"h1.0": relative L2, ..},
        "differing": {"h1.0": fraction of elements that differ at all, ..}} of the kernel against the mirrored reference."""
        q = {"l2": {}, "max": {}, "stage": {}, "differing": {}}
        for nm in self.c.names:
            got = self.c.gradient(nm)
            q["l2"][nm], q["max"][nm] = W.rel_l2(got, self.gref[nm]), W.max_rel(got, self.gref[nm])
        for s in STAGES:
            for t in range(2):
                got, ref = self.stage(s, t)
                q["stage"]["%s.%d" % (s, t)] = W.rel_l2(got, ref)
                q["differing"]["%s.%d" % (s, t)] = float((got != ref).double().mean())
        return q


@functools.lru_cache(maxsize=None)
def _run(key, seed=W.SEEDS[0]):
    return _Run(key, seed)


# ------------------------------------------------------------------------------------------------ 1. packing, bit-exact
@pytest.mark.parametrize("key", KEYS)
def test_wide_packing_is_bit_exact(key):
    """wpk of both trunks equals ppo_wide_ref64.packed_reference block by block (W1 | W2 | W2^T | W3 | W3^T, read through unfrag,
    compared as int16 with torch.equal: zero error allowed), xbT rows < D equal round(obs)^T and rows D .. Dp are zero; rows
    Dp .. round32(Dp) of xbT are never read and only the guard behind the array is asserted."""
    r = _run(key)
    c = r.c
    B, D, H1, H2, A = c.dims
    par = dict(c.pol.named_parameters())
    for t, (pre, head) in enumerate(W.TRUNKS):
        At = A if t == 0 else 1
        ref = W.packed_reference((par[pre + ".0.weight"], par[pre + ".2.weight"], par[head + ".weight"]), D, H1, H2, At)
        wpk, off = c.bf["wpk%d" % t][1], 0
        for blk, (N, K) in zip(ref, ((H1, c.Dp), (H2, H1), (H1, H2), (32, H2), (H2, 32))):
            assert blk.shape == (N, K)
            assert torch.equal(W.unfrag(wpk[off:off + N * K], N, K), blk.view(torch.int16)), (key, t, N, K)
            off += N * K
        assert off == c.npk
    xref = torch.zeros(c.Dp, B, device=DEV, dtype=torch.bfloat16)
    xref[:D] = c.batch[0].to(torch.bfloat16).t()
    assert torch.equal(c.T("xbT", c.N32)[:c.Dp], xref.view(torch.int16))
    assert torch.equal(xref[:D].double(), r.inter["xb"].t())
    assert not c.guards_ok()


# ------------------------------------------------------------------------------------------------ 2. per-stage intermediates
@pytest.mark.parametrize("key", KEYS)
def test_wide_stage_intermediates_match_the_mirrored_reference(key):
    """h1T, h2T, dz3T, dz2T, dz1T of both trunks, un-fragmented, against the reference's arrays: relative L2 within
    BOUNDS[key]["stage"] (module docstring: 10 x the CPU self-distance, <= 6.2e-3, unmeasured on the device), at most 5 % of a
    stage's elements differ at all from the reference's bf16 value (bf16 ties decided differently by fp32 and fp64; CPU
    self-distance <= 1.6 %), dz3T rows >= A (policy) / >= 1 (value) exactly zero.  A stage that is O(1) off localises a bug to
    that stage."""
    r = _run(key)
    B, D, H1, H2, A = r.c.dims
    q = r.quantities()
    for t in range(2):
        dz3 = r.c.T("dz3T%d" % t, 32)
        assert not bool(dz3[A if t == 0 else 1:].any()), (key, t)
    for sk in q["stage"]:
        _note("%s differing %s" % (key, sk), q["differing"][sk], MAX_DIFFERING)
        bound = W.BOUNDS[key]["stage"][sk]
        _note("%s stage rel L2 %s" % (key, sk), q["stage"][sk], bound)
    for sk in q["stage"]:
        assert q["differing"][sk] <= MAX_DIFFERING, (key, sk, q["differing"][sk])
        assert q["stage"][sk] <= W.BOUNDS[key]["stage"][sk], (key, sk, q["stage"][sk])


# ------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("key", KEYS)
def test_wide_gradients_match_the_mirrored_reference(key):
    """Every parameter gradient and each single g_log_std entry against the mirrored fp64 reference: relative L2 within
    BOUNDS[key]["l2"][name] and max-abs over the tensor's largest entry within BOUNDS[key]["max"][name] (module docstring: 10 x
    the CPU self-distance; relative L2 <= 5.9e-3, max-abs <= 2e-2; unmeasured on the device).  Without folds (first shape) the
    arena starts from a known non-zero pattern and the result is pattern + gradient."""
    r = _run(key)
    c = r.c
    assert torch.isfinite(c.arena).all()
    q = r.quantities()
    for nm in c.names:
        _note("%s rel L2 d/d %s" % (key, nm), q["l2"][nm], W.BOUNDS[key]["l2"][nm])
        _note("%s max-abs d/d %s" % (key, nm), q["max"][nm], W.BOUNDS[key]["max"][nm])
    for nm in c.names:
        assert float(r.gref[nm].abs().max()) > 0, nm
        assert q["l2"][nm] <= W.BOUNDS[key]["l2"][nm], (key, nm, q["l2"][nm])
        assert q["max"][nm] <= W.BOUNDS[key]["max"][nm], (key, nm, q["max"][nm])
    gl, ref = c.gradient("log_std"), r.gref["log_std"]
    assert gl.numel() == c.dims[4]
    assert bool(((gl - ref).abs() <= W.BOUNDS[key]["max"]["log_std"] * float(ref.abs().max())).all())


# ------------------------------------------------------------------------------------------------ 4. out8, 5. folds, 6. guards
@pytest.mark.parametrize("key", KEYS)
def test_wide_out8_folds_and_guards(key):
    """All eight out8 entries by _check_out8's rules against the MIRRORED reference's out8 (loss terms 2e-5, approx_kl 5e-5, clip
    fraction exact: no row lies within 1e-2 of a clip boundary), the advantage statistics in out8[6, 7] and stats8[0, 1] against
    fp64 (1e-5 relative; exactly (0, 1) with normalize off).  Folds: the NaN arena is finite afterwards, the floats behind
    zero_floats are untouched, adam_state2 goes (x, n) -> (0, n + 1), loss_acc (s, k) -> (s + out8[0], k + 1) bit-exactly; the
    call without folds passes NULL for adam_state2 / loss_acc.  The guard behind every array, `part` included, is intact."""
    r = _run(key)
    c = r.c
    B = c.dims[0]
    out8, stats8 = c.f32["out8"][1], c.f32["stats8"][1]
    assert torch.isfinite(out8).all()
    _check_out8(out8, r.ref8, r.ratio64, c.clip, B)
    assert int((((r.ratio64 - 1).abs() - c.clip).abs() < 1e-3).sum()) == 0
    adv = c.batch[2].double()
    if c.normalize:
        am, inv = float(adv.mean()), 1.0 / (float(adv.std()) + 1e-8)
        assert 0.05 < float(r.ref8[5]) < 0.95
        for got in (stats8[:2], out8[6:8]):
            assert abs(float(got[0]) - am) < 1e-5 * max(1.0, abs(am)) and abs(float(got[1]) - inv) < 1e-5 * inv
    else:
        assert stats8[:2].tolist() == [0.0, 1.0] and out8[6:8].tolist() == [0.0, 1.0]
    assert torch.equal(stats8[:2], out8[6:8])
    assert torch.isfinite(c.arena).all()
    if c.folds:
        assert c.st.zero_floats == c.n and _guard_ok(c.arena_buf, c.arena)
        assert c.f32["adam_state2"][1].tolist() == [0.0, 8.0]
        la = c.f32["loss_acc"][1]
        assert torch.equal(la[0], torch.tensor(1.25, device=DEV) + out8[0]) and float(la[1]) == 4.0
    else:
        assert c.st.zero_ptr is None and c.st.adam_state2 is None and c.st.loss_acc is None
    assert torch.isfinite(c.f32["part"][1].view(-1, 40)[:, :36]).all()          # 36 of a row's 40 floats are written
    assert c.guards_ok() == []


# ------------------------------------------------------------------------------------------------ reproducibility
def test_wide_weight_gradients_are_bit_reproducible_without_split_k():
    """The source's claim ("with splitk == 1 a plain store: no atomics, bit-reproducible gradients"): at (1024,512), D 67, A 28,
    B 256 every weight-gradient job has split-K 1 (otiles x itiles x 2 exceeds the wanted workgroups for all six), so two calls on
    the same inputs, each with fresh scratch, give bit-identical gW for all six layers.  The bias gradients go through atomics
    and are held to the gradient bound only (test_wide_gradients_match_the_mirrored_reference)."""
    key = "1024x512-d67-a28-b256"
    a, b = _run(key).c, _Call(key, W.SEEDS[0])
    assert b.launch() == 0
    for x, y in zip(a.batch, b.batch):
        assert torch.equal(x, y)
    for nm in a.names:
        if nm.endswith(".weight"):
            assert torch.equal(a.g[nm], b.g[nm]), nm
    assert b.guards_ok() == []


# ------------------------------------------------------------------------------------------------ the -22 paths (no launch)
@pytest.mark.parametrize("field,value", [("B", 96), ("H1", 384), ("H2", 192), ("D", 113), ("A", 33)])
def test_wide_unsupported_shape_is_refused_before_any_launch(field, value):
    """dm_ppo_wide_supported says 0 and dm_ppo_wide_grad returns -22 for B = 96 (not a multiple of 64), H1 = 384, H2 = 192,
    D = 113, A = 33; an argument check: every guarded output and scratch array still holds its fill pattern."""
    c = _Call("256x128-d85-a23-b1024", W.SEEDS[0])
    dims = dict(zip(("B", "D", "H1", "H2", "A"), c.dims))
    dims[field] = value
    assert _lib().dm_ppo_wide_supported(dims["B"], dims["D"], dims["H1"], dims["H2"], dims["A"]) == 0
    setattr(c.st, field, value)
    assert c.launch() == -22
    assert c.untouched()


def test_wide_null_required_pointer_is_refused_before_any_launch():
    """Each required pointer of DmPpoWideStep set to NULL in turn (and a NULL step): -22, nothing launched, every guarded output
    and scratch array still holds its fill pattern.  zero_ptr, adam_state2 and loss_acc are optional and not in the list."""
    c = _Call("256x128-d1-a1-b64", W.SEEDS[0])
    assert _lib().dm_ppo_wide_grad(None, _stream()) == -22
    n = 0
    for f in ("obs", "act", "adv", "ret", "old_logp", "log_std", "g_log_std", "xbT", "part", "stats8", "out8"):
        keep = getattr(c.st, f)
        setattr(c.st, f, None)
        assert c.launch() == -22, f
        setattr(c.st, f, keep)
        n += 1
    for f in ("wpk", "h1T", "dz1T", "h2T", "dz2T", "dz3T"):
        for t in range(2):
            keep = getattr(c.st, f)[t]
            getattr(c.st, f)[t] = None
            assert c.launch() == -22, (f, t)
            getattr(c.st, f)[t] = keep
            n += 1
    for f in ("W", "b", "gW", "gb"):
        for t in range(2):
            for l in range(3):
                keep = getattr(c.st, f)[t][l]
                getattr(c.st, f)[t][l] = None
                assert c.launch() == -22, (f, t, l)
                getattr(c.st, f)[t][l] = keep
                n += 1
    assert n == 11 + 12 + 24
    assert c.untouched()
