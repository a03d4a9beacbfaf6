"""dm_ppo_wide3_grad (csrc/dm_ppo_wide3.hip, the bf16x3 learner) called directly through DmPpoWide3Step, with buffers the test owns,
against the fp64 reference that splits where the kernel splits (tests/ppo_wide3_ref64.py) and against the unrounded fp64 chain.

Shapes: the six of ppo_wide_ref64.SHAPES (table in test_ppo_wide_kernel_gpu.py).  The new tiling adds one branch, the number of
256-column chunks of layer 1, and the six shapes reach every value of it: H1 = 256 (one chunk), 512 (two), 768 (three, an odd
count), 1024 (four); a chunk is never uneven (H1 % 256 == 0).  They also reach the waves that own no layer-2 tile (H2 = 128: two
of eight waves own tiles; 256: four; 384: six; 512: all).

Every output and scratch array is a view at the front of a buffer filled with NaN (fp32) or 0x7FC0 (bf16) with a guard region
behind it.  Bounds: ppo_wide3_ref64.BOUNDS (10 x the CPU self-distance of the mirrored chain, module docstring there), and
ppo_wide3_ref64.UNROUNDED_BOUND = 1e-4 for every gradient against the unrounded fp64 chain.  Run with -s for the "measured / bound /
margin" lines.
"""
import functools

import pytest
import torch

import ppo_wide_ref64 as W
import ppo_wide3_ref64 as W3
from kernel_helpers import DEV, check_out8, guard_ok as _guard_ok, lib as _lib, note, stream as _stream
from wide_call import WideCall

pytestmark = pytest.mark.gpu

KEYS = list(W.SHAPES)
MAX_DIFFERING = 0.05     # at most this fraction of a stage's hi-plane elements may differ from the reference's
STAGES = ("h1", "h2", "dz3", "dz2", "dz1")

_note = functools.partial(note, width=46)
_check_out8 = functools.partial(check_out8, width=46)


class _Call(WideCall):
    """The buffers of one dm_ppo_wide3_grad call and its DmPpoWide3Step.  self.plane[name] = elements of one plane of the array."""

    entry, packed_elems, supported, step_cls = "dm_ppo_wide3_grad", "dm_ppo_wide3_packed_elems", "dm_ppo_wide3_supported", "DmPpoWide3Step"
    planes, ref = 2, W3

    def planes_of(self, name):
        """(hi, lo) flat int16 planes of a two-plane array."""
        v, n = self.bf[name][1], self.plane[name]
        return v[:n], v[n:2 * n]

    def T(self, name, N):
        """(hi, lo) of a transposed scratch array [N][B], un-fragmented, as int16."""
        return tuple(W.unfrag(p, N, self.dims[0]) for p in self.planes_of(name))


class _Run:
    """One launch, the mirrored reference and the unrounded fp64 chain of the same minibatch."""

    def __init__(self, key, seed):
        c = self.c = _Call(key, seed)
        assert c.launch() == 0
        kw = dict(clip_range=c.clip, vf_coef=c.vf, ent_coef=c.ent, normalize=c.normalize)
        self.loss, self.ref8, self.gref, self.inter = W3.wide3_chain(c.P, c.batch, **kw)
        self.gexact = W3.unrounded_chain(c.P, c.batch, **kw)[2]
        self.ratio64 = torch.exp(W3.log_ratio(c.P, c.batch))

    def stage(self, s, t):
        """((hi, lo) of the kernel's array [N][B] as fp64, the reference's (hi, lo) [N][B]) of stage s, trunk t; dz3: the live head
        rows only."""
        c = self.c
        B, D, H1, H2, A = c.dims
        N = {"h1": H1, "dz1": H1, "h2": H2, "dz2": H2, "dz3": 32}[s]
        got = tuple(p.view(torch.bfloat16).double() for p in c.T("%sT%d" % (s, t), N))
        ref = tuple(p.t() for p in self.inter[s][t])
        if s == "dz3":
            live = A if t == 0 else 1
            got, ref = tuple(p[:live] for p in got), tuple(p[:live] for p in ref)
        return got, ref

    @functools.lru_cache(maxsize=None)
    def quantities(self):
        """{"l2" / "max": per gradient against the mirrored reference; "xl2" / "xmax": against the unrounded fp64 chain; "stage":
        relative L2 of hi + lo; "differing": fraction of hi-plane elements that differ from the reference's}."""
        q = {"l2": {}, "max": {}, "xl2": {}, "xmax": {}, "stage": {}, "differing": {}}
        for nm in self.c.names:
            got = self.c.gradient(nm)
            q["l2"][nm], q["max"][nm] = W.rel_l2(got, self.gref[nm]), W.max_rel(got, self.gref[nm])
            q["xl2"][nm], q["xmax"][nm] = W.rel_l2(got, self.gexact[nm]), W.max_rel(got, self.gexact[nm])
        for s in STAGES:
            for t in range(2):
                got, ref = self.stage(s, t)
                q["stage"]["%s.%d" % (s, t)] = W.rel_l2(W3.val(got), W3.val(ref))
                q["differing"]["%s.%d" % (s, t)] = float((got[0] != ref[0]).double().mean())
        return q


@functools.lru_cache(maxsize=None)
def _run(key, seed=W.SEEDS[0]):
    return _Run(key, seed)


# ------------------------------------------------------------------------------------------------ 1. packing, bit-exact
@pytest.mark.parametrize("key", KEYS)
def test_wide3_packing_is_bit_exact(key):
    """Both planes of wpk of both trunks equal ppo_wide3_ref64.packed_reference block by block (W1 | W2 | W2^T | W3 | W3^T, read
    through unfrag, compared as int16 with torch.equal), plane 1 starting at the one-plane element count; both planes of xbT rows
    < D equal the split of obs^T and rows D .. Dp are zero."""
    r = _run(key)
    c = r.c
    B, D, H1, H2, A = c.dims
    par = dict(c.pol.named_parameters())
    for t, (pre, head) in enumerate(W.TRUNKS):
        At = A if t == 0 else 1
        ref = W3.packed_reference((par[pre + ".0.weight"], par[pre + ".2.weight"], par[head + ".weight"]), D, H1, H2, At)
        for plane, blocks in zip(c.planes_of("wpk%d" % t), ref):
            off = 0
            for blk, (N, K) in zip(blocks, ((H1, c.Dp), (H2, H1), (H1, H2), (32, H2), (H2, 32))):
                assert blk.shape == (N, K)
                assert torch.equal(W.unfrag(plane[off:off + N * K], N, K), blk.view(torch.int16)), (key, t, N, K)
                off += N * K
            assert off == c.npk // 2
    hi, lo = W3.round_split(c.batch[0])
    for plane, x, rx in zip(c.T("xbT", c.N32), (hi, lo), r.inter["xb"]):
        xref = torch.zeros(c.Dp, B, device=DEV, dtype=torch.bfloat16)
        xref[:D] = x.to(torch.bfloat16).t()
        assert torch.equal(plane[:c.Dp], xref.view(torch.int16))
        assert torch.equal(xref[:D].double(), rx.t())
    assert not c.guards_ok()


# ------------------------------------------------------------------------------------------------ 2. per-stage intermediates
@pytest.mark.parametrize("key", KEYS)
def test_wide3_stage_intermediates_match_the_mirrored_reference(key):
    """h1T, h2T, dz3T, dz2T, dz1T of both trunks, reconstructed as hi + lo, against the reference's: relative L2 within
    BOUNDS[key]["stage"]; the hi plane differs from the reference's in at most 5 % of a stage's elements; both planes of dz3T rows
    >= A (policy) / >= 1 (value) exactly zero."""
    r = _run(key)
    B, D, H1, H2, A = r.c.dims
    q = r.quantities()
    for t in range(2):
        for plane in r.c.T("dz3T%d" % t, 32):
            assert not bool(plane[A if t == 0 else 1:].any()), (key, t)
    for sk in q["stage"]:
        _note("%s differing %s" % (key, sk), q["differing"][sk], MAX_DIFFERING)
        _note("%s stage rel L2 %s" % (key, sk), q["stage"][sk], W3.BOUNDS[key]["stage"][sk])
    for sk in q["stage"]:
        assert q["differing"][sk] <= MAX_DIFFERING, (key, sk, q["differing"][sk])
        assert q["stage"][sk] <= W3.BOUNDS[key]["stage"][sk], (key, sk, q["stage"][sk])


# ------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("key", KEYS)
def test_wide3_gradients_match_the_mirrored_reference(key):
    """Every parameter gradient and each single g_log_std entry against the mirrored fp64 reference: relative L2 within
    BOUNDS[key]["l2"][name] and max-abs over the tensor's largest entry within BOUNDS[key]["max"][name]."""
    r = _run(key)
    c = r.c
    assert torch.isfinite(c.arena).all()
    q = r.quantities()
    for nm in c.names:
        _note("%s rel L2 d/d %s" % (key, nm), q["l2"][nm], W3.BOUNDS[key]["l2"][nm])
        _note("%s max-abs d/d %s" % (key, nm), q["max"][nm], W3.BOUNDS[key]["max"][nm])
    for nm in c.names:
        assert float(r.gref[nm].abs().max()) > 0, nm
        assert q["l2"][nm] <= W3.BOUNDS[key]["l2"][nm], (key, nm, q["l2"][nm])
        assert q["max"][nm] <= W3.BOUNDS[key]["max"][nm], (key, nm, q["max"][nm])
    gl, ref = c.gradient("log_std"), r.gref["log_std"]
    assert gl.numel() == c.dims[4]
    assert bool(((gl - ref).abs() <= W3.BOUNDS[key]["max"]["log_std"] * float(ref.abs().max())).all())


@pytest.mark.parametrize("key", KEYS)
def test_wide3_gradients_are_within_1e_4_of_the_unrounded_fp64_chain(key):
    """The point of the learner: every gradient within 1e-4, relative L2 and max-abs over the largest entry, of the fp64 chain
    with no rounding at all (the bound of the project's fused fp32 [256,128] learner; the bf16 kernel sits near 1e-2)."""
    r = _run(key)
    q = r.quantities()
    for nm in r.c.names:
        _note("%s unrounded rel L2 d/d %s" % (key, nm), q["xl2"][nm], W3.UNROUNDED_BOUND)
        _note("%s unrounded max-abs d/d %s" % (key, nm), q["xmax"][nm], W3.UNROUNDED_BOUND)
    for nm in r.c.names:
        assert q["xl2"][nm] <= W3.UNROUNDED_BOUND, (key, nm, q["xl2"][nm])
        assert q["xmax"][nm] <= W3.UNROUNDED_BOUND, (key, nm, q["xmax"][nm])


# ------------------------------------------------------------------------------------------------ 4. out8, 5. folds, 6. guards
@pytest.mark.parametrize("key", KEYS)
def test_wide3_out8_folds_and_guards(key):
    """All eight out8 entries by check_out8's rules against the mirrored reference's out8, the advantage statistics in out8[6, 7]
    and stats8[0, 1] against fp64; the folds (arena cleared, adam_state2 (x, n) -> (0, n + 1), loss_acc (s, k) -> (s + out8[0],
    k + 1) bit-exactly); the call without folds passes NULL for them.  The guard behind every array is intact."""
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
def test_wide3_weight_gradients_are_bit_reproducible_without_split_k():
    """At (1024,512), D 67, A 28, B 256 every weight-gradient job has split-K 1, so two calls on the same inputs, each with fresh
    scratch, give bit-identical gW for all six layers."""
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
def test_wide3_unsupported_shape_is_refused_before_any_launch(field, value):
    """dm_ppo_wide3_supported says 0 and dm_ppo_wide3_grad returns -22 for B = 96, H1 = 384, H2 = 192, D = 113, A = 33; every
    guarded output and scratch array still holds its fill pattern."""
    c = _Call("256x128-d85-a23-b1024", W.SEEDS[0])
    dims = dict(zip(("B", "D", "H1", "H2", "A"), c.dims))
    dims[field] = value
    assert _lib().dm_ppo_wide3_supported(dims["B"], dims["D"], dims["H1"], dims["H2"], dims["A"]) == 0
    setattr(c.st, field, value)
    assert c.launch() == -22
    assert c.untouched()


def test_wide3_null_required_pointer_is_refused_before_any_launch():
    """Each required pointer of DmPpoWide3Step set to NULL in turn (and a NULL step): -22, nothing launched, every guarded output
    and scratch array still holds its fill pattern.  zero_ptr, adam_state2 and loss_acc are optional and not in the list."""
    c = _Call("256x128-d1-a1-b64", W.SEEDS[0])
    assert _lib().dm_ppo_wide3_grad(None, _stream()) == -22
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
