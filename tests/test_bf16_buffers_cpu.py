"""bf16 rollout buffers (``PPO(buffer_dtype=torch.bfloat16)``) without a GPU: the four new entry points are declared, listed and
exported next to the old ones, refuse bad arguments with -22 before anything touches a device, and the CPU path of ``PPO`` is the
plain loop it always was."""
import ctypes as C
import os
import re

import torch

from sac_helpers import BanditEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dm_policy_forward_bf16", "dm_rollout_store_bf16", "dm_ppo_gather_bf16", "dm_flat_adam_step_gather_bf16")
OLD = ("dm_policy_forward", "dm_rollout_store", "dm_ppo_gather", "dm_flat_adam_step_gather", "dm_flat_adam_step", "dm_flat_adam_update",
       "dm_policy_sample", "dm_policy_pack", "dm_policy_packed_floats", "dm_rollout_finish")
X = C.c_void_p(0x1000)      # a non-null pointer that is never followed: every call below must return before any launch


def _lib():
    from deepmimic_mujoco_amd import _lib
    return _lib, _lib.load_library()


def test_new_entry_points_are_declared_listed_and_exported_beside_the_old_ones():
    mod, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "deepmimic_hip.h")).read()
    declared = set(re.findall(r"\b(dm_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW + OLD:
        assert name in declared, name
        assert name in mod.EXPORTS, name
        assert getattr(L, name) is not None
    assert "DmGatherSpecBf16" in hdr and "typedef struct DmGatherSpec {" in hdr
    # the new spec mirrors the old one's layout (14 pointers / ints in the same places)
    assert C.sizeof(mod.DmGatherSpecBf16) == C.sizeof(mod.DmGatherSpec)
    assert [f[0] for f in mod.DmGatherSpecBf16._fields_] == [f[0] for f in mod.DmGatherSpec._fields_]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integ, name


def _forward_args(**kw):
    a = dict(obs=X, N=64, D=67, H1=256, H2=128, A=28, pi_packed=X, pi_b1=X, pi_b2=X, pi_b3=X, vf_packed=X, vf_b1=X, vf_b2=X, vf_b3=X,
             log_std=X, seed=C.c_uint64(1), counter=X, draw_offset=C.c_uint32(0), deterministic=0, lo=X, hi=X, mean_out=None, act=X,
             act_env=X, logp=X, val=X, obs_copy=None, stream=None)
    a.update(kw)
    return list(a.values())


def test_policy_forward_bf16_rejects_bad_arguments():
    _, L = _lib()
    for bad in (dict(obs=None), dict(act=None), dict(act_env=None), dict(logp=None), dict(val=None), dict(counter=None), dict(pi_packed=None),
                dict(N=0), dict(N=-3), dict(A=33), dict(H1=100), dict(pi_packed=C.c_void_p(0x1004))):
        assert L.dm_policy_forward_bf16(*_forward_args(**bad)) == -22, bad
        if "pi_packed" not in bad or bad["pi_packed"] is None:
            assert L.dm_policy_forward(*_forward_args(**bad)) == -22, bad       # the old entry point answers alike


def _store_args(**kw):
    a = dict(N=8, D=67, A=28, last_obs=X, act=X, val=X, logp=X, rew=X, done=X, new_obs=X, b_obs=X, b_act=X, b_val=X, b_logp=X, b_rew=X,
             b_done=X, last_obs_out=X, counter=None, stream=None)
    a.update(kw)
    return list(a.values())


def test_rollout_store_bf16_rejects_bad_arguments():
    _, L = _lib()
    for bad in (dict(N=0), dict(N=-1), dict(last_obs=None), dict(act=None), dict(b_obs=None), dict(b_act=None), dict(b_done=None),
                dict(last_obs_out=None), dict(new_obs=None)):
        assert L.dm_rollout_store_bf16(*_store_args(**bad)) == -22, bad


def _gather_args(**kw):
    a = dict(idx=X, B=16, obs=X, D=67, act=X, A=28, adv=X, ret=X, logp=X, o_obs=X, o_act=X, o_adv=X, o_ret=X, o_logp=X, stream=None)
    a.update(kw)
    return list(a.values())


def test_gather_bf16_rejects_bad_arguments():
    _, L = _lib()
    for bad in (dict(B=0), dict(B=-5), dict(idx=None), dict(obs=None), dict(act=None), dict(logp=None), dict(o_obs=None), dict(o_logp=None),
                dict(D=0), dict(D=1025), dict(A=1025)):
        assert L.dm_ppo_gather_bf16(*_gather_args(**bad)) == -22, bad


def test_flat_adam_step_gather_bf16_rejects_bad_arguments():
    mod, L = _lib()

    def call(spec=True, n=1000, state2_floats=1026, **kw):
        gs = mod.DmGatherSpecBf16()
        vals = dict(idx=0x1000, B=16, D=67, A=28, obs=0x1000, act=0x1000, adv=0x1000, ret=0x1000, logp=0x1000, o_obs=0x1000, o_act=0x1000,
                    o_adv=0x1000, o_ret=0x1000, o_logp=0x1000)
        vals.update(kw)
        for k, v in vals.items():
            setattr(gs, k, v)
        return L.dm_flat_adam_step_gather_bf16(X, X, X, X, n, 4e-4, 0.9, 0.999, 1e-5, 0.5, 1.0, X, state2_floats, 1,
                                               C.byref(gs) if spec else None, None)

    assert call(spec=False) == -22                       # the spec is what this entry point is for
    for bad in (dict(B=0), dict(B=-1), dict(idx=None), dict(obs=None), dict(act=None), dict(adv=None), dict(o_obs=None), dict(o_act=None),
                dict(D=0), dict(A=0), dict(D=1025), dict(A=2000)):
        assert call(**bad) == -22, bad
    assert call(n=0) == -22 and call(state2_floats=2) == -22


def test_cpu_ppo_with_bf16_buffers_reports_and_runs_the_plain_path():
    """CPU behaviour is unchanged: buffer_dtype only narrows what the plain loop stores, and rollout_path() says "plain"."""
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        from deepmimic_mujoco_amd.ppo import PPO
        env = BanditEnv(16, 9, 3, seed=5)
        ppo = PPO(env, net_arch=(32, 32), n_steps=4, batch_size=32, n_epochs=1, seed=2, buffer_dtype=dt)
        assert not ppo._fused_rollout_ok() and not ppo._fused_policy_ok()
        assert ppo.rollout_path() == "plain"
        torch.manual_seed(7)
        buf = ppo.collect_rollouts()
        assert buf["obs"].dtype == dt and buf["act"].dtype == dt
        assert all(buf[k].dtype == torch.float32 for k in ("rew", "done", "val", "logp", "adv", "ret"))
        res[dt] = buf
    a, b = res[torch.float32], res[torch.bfloat16]
    for k in ("rew", "done", "val", "logp", "adv", "ret"):
        assert torch.equal(a[k], b[k]), k                # nothing but the stored obs / act sees the storage type
    assert torch.equal(b["obs"].view(torch.int16), a["obs"].to(torch.bfloat16).view(torch.int16))
    assert torch.equal(b["act"].view(torch.int16), a["act"].to(torch.bfloat16).view(torch.int16))


def test_gather_storage_names_the_kernel_for_a_buffer():
    from deepmimic_mujoco_amd.ppo import gather_storage
    f = lambda od, ad=None, x=torch.float32: dict(obs=torch.zeros(2, 3, dtype=od), act=torch.zeros(2, 2, dtype=ad or od),
                                                  adv=torch.zeros(2, dtype=x), ret=torch.zeros(2), logp=torch.zeros(2))
    assert gather_storage(f(torch.float32)) == "fp32" and gather_storage(f(torch.bfloat16)) == "bf16"
    assert gather_storage(f(torch.float16)) is None and gather_storage(f(torch.bfloat16, torch.float32)) is None
    assert gather_storage(f(torch.bfloat16, x=torch.float64)) is None
    assert gather_storage(f(torch.bfloat16), torch.zeros(2, dtype=torch.int32)) is None
    assert gather_storage(f(torch.bfloat16), torch.zeros(2, dtype=torch.int64)) == "bf16"
