"""The harness the kernel tests of the two wide learners share (test_ppo_wide_kernel_gpu.py: dm_ppo_wide_grad, one bf16 plane per
scratch array; test_ppo_wide3_kernel_gpu.py: dm_ppo_wide3_grad, two planes): the policy, the known arena pattern and the buffers
and step struct of one call.  A plain module: importing it touches no GPU."""
import ctypes as C

import torch
import torch.nn as nn

import ppo_ref64 as R
import ppo_wide_ref64 as W
from kernel_helpers import BF16_NAN, DEV, guard_ok, guard_ok_bf16, guarded, guarded_bf16, lib, stream


def policy(arch, D, A, seed=13):
    """SB3-style init (MlpPolicy: orthogonal weights), biases N(0, 0.1) so that a wrong bias shows, log_std += 0.1 N(0, 1)."""
    from deepmimic_mujoco_amd.ppo import MlpPolicy
    torch.manual_seed(seed)
    pol = MlpPolicy(obs_dim=D, act_dim=A, net_arch=arch).to(DEV)
    with torch.no_grad():
        pol.log_std.add_(0.1 * torch.randn(A, device=DEV))
        for m in pol.modules():
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
    return pol


def pattern(n):
    """The known non-zero content of the gradient arena of the call without folds (exact in fp32, of a gradient's size)."""
    return ((torch.arange(n, device=DEV) % 7) + 1).float() * 2.0 ** -13


class WideCall:
    """The buffers of one call of a wide learner and its step struct.  A subclass names the entry point (`entry`), its
    `packed_elems` / `supported` calls, the step struct of deepmimic_mujoco_amd._lib (`step_cls`), the planes per bf16 scratch
    array (`planes`) and the reference module that makes the minibatch (`ref`).  self.plane[name] = elements of one plane."""

    entry = packed_elems = supported = step_cls = ref = None
    planes = 1

    def __init__(self, key, seed):
        arch, D, A, B, normalize, ent, folds = W.SHAPES[key]
        H1, H2 = arch
        L = lib()
        self.key, self.dims, self.normalize, self.ent, self.folds = key, (B, D, H1, H2, A), normalize, ent, folds
        self.clip, self.vf = 0.2, 0.5
        assert getattr(L, self.supported)(B, D, H1, H2, A) == 1
        self.Dp = int(L.dm_ppo_wide_dp(D))
        assert self.Dp == W.dp(D)
        self.npk = int(getattr(L, self.packed_elems)(D, H1, H2))
        assert self.npk == self.planes * (H1 * self.Dp + 2 * H1 * H2 + 64 * H2) == self.planes * int(L.dm_ppo_wide_packed_elems(D, H1, H2))
        self.pol = policy(arch, D, A)
        self.P = R.params64(self.pol, DEV)
        self.batch = self.ref.make_batch(self.P, D, A, B, seed, self.clip)
        self.names = [n for n, _ in self.pol.named_parameters()]
        par = dict(self.pol.named_parameters())
        # gradients: one arena in named_parameters order (NaN with the folds, which clear it; a known pattern without)
        n = sum(p.numel() for p in par.values())
        self.n = n
        self.arena_buf, self.arena = guarded(n)
        if not folds:
            self.arena.copy_(pattern(n))
        self.g, off = {}, 0
        for nm in self.names:
            self.g[nm] = self.arena[off:off + par[nm].numel()].view_as(par[nm])
            off += par[nm].numel()
        N32 = (self.Dp + 31) // 32 * 32
        self.N32 = N32
        self.plane = {"xbT": N32 * B}
        for t in range(2):
            self.plane["wpk%d" % t] = self.npk // self.planes
            self.plane["h1T%d" % t] = self.plane["dz1T%d" % t] = H1 * B
            self.plane["h2T%d" % t] = self.plane["dz2T%d" % t] = H2 * B
            self.plane["dz3T%d" % t] = 32 * B
        self.bf = {k: guarded_bf16(self.planes * v) for k, v in self.plane.items()}
        self.f32 = {"part": guarded(2 * (B // 32) * 40), "stats8": guarded(8), "out8": guarded(8)}
        if folds:
            self.f32["adam_state2"], self.f32["loss_acc"] = guarded(2), guarded(2)
            self.f32["adam_state2"][1].copy_(torch.tensor([3.5, 7.0]))
            self.f32["loss_acc"][1].copy_(torch.tensor([1.25, 3.0]))
        from deepmimic_mujoco_amd import _lib
        st = getattr(_lib, self.step_cls)()
        st.B, st.D, st.H1, st.H2, st.A = B, D, H1, H2, A
        st.normalize_advantage, st.clip_range, st.vf_coef, st.ent_coef = int(normalize), self.clip, self.vf, ent
        st.obs, st.act, st.adv, st.ret, st.old_logp = (t.data_ptr() for t in self.batch)
        st.log_std, st.g_log_std = par["log_std"].data_ptr(), self.g["log_std"].data_ptr()
        for t, (pre, head) in enumerate(W.TRUNKS):
            for l, nm in enumerate((pre + ".0", pre + ".2", head)):
                st.W[t][l], st.b[t][l] = par[nm + ".weight"].data_ptr(), par[nm + ".bias"].data_ptr()
                st.gW[t][l], st.gb[t][l] = self.g[nm + ".weight"].data_ptr(), self.g[nm + ".bias"].data_ptr()
            for k in ("wpk", "h1T", "dz1T", "h2T", "dz2T", "dz3T"):
                getattr(st, k)[t] = self.bf["%s%d" % (k, t)][1].data_ptr()
        st.xbT = self.bf["xbT"][1].data_ptr()
        st.part, st.stats8, st.out8 = (self.f32[k][1].data_ptr() for k in ("part", "stats8", "out8"))
        if folds:
            st.zero_ptr, st.zero_floats = self.arena.data_ptr(), n
            st.adam_state2, st.loss_acc = self.f32["adam_state2"][1].data_ptr(), self.f32["loss_acc"][1].data_ptr()
        self.st = st

    def launch(self, st=None):
        """One call on the shared stream, one synchronize; returns the return code."""
        rc = getattr(lib(), self.entry)(C.byref(self.st if st is None else st), stream())
        torch.cuda.synchronize()
        return rc

    def guards_ok(self):
        bad = [k for k, (b, v) in self.bf.items() if not guard_ok_bf16(b, v)]
        bad += [k for k, (b, v) in self.f32.items() if not guard_ok(b, v)]
        if not guard_ok(self.arena_buf, self.arena):
            bad.append("gradient arena")
        return bad

    def untouched(self):
        """Every output and scratch array still holds what it was filled with."""
        ok = all(bool((v == BF16_NAN).all()) for _, v in self.bf.values())
        ok = ok and all(bool(torch.isnan(self.f32[k][1]).all()) for k in ("part", "stats8", "out8"))
        if self.folds:
            ok = ok and self.f32["adam_state2"][1].tolist() == [3.5, 7.0] and self.f32["loss_acc"][1].tolist() == [1.25, 3.0]
            return ok and bool(torch.isnan(self.arena).all()) and not self.guards_ok()
        return ok and torch.equal(self.arena, pattern(self.n)) and not self.guards_ok()

    def gradient(self, nm):
        g = self.g[nm].double()
        if not self.folds:
            off = self.g[nm].data_ptr() - self.arena.data_ptr()
            g = g - pattern(self.n)[off // 4:off // 4 + g.numel()].view_as(g).double()
        return g
