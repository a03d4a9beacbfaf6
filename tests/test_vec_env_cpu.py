"""The batch-env base (deepmimic_mujoco_amd/vec_env.py) on a CPU, driven through a fake engine factory.

The fake engine is plain Python over CPU torch tensors: it records its calls and, on ``step``, writes values that encode the
global env index and the step number, so every number ``step_wait`` hands out can be traced to the engine and row that wrote it.
Both (obs, terms, actions) shapes of the package run: (67, 5, 28) with ``LazyInfos`` and (98, 8, 23) with ``_LazyCombinedInfos``.
"""
import types

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib, g1
from deepmimic_mujoco_amd.combined_env import _LazyCombinedInfos, _combined_info
from deepmimic_mujoco_amd.deepmimic_env import LazyInfos, _make_info
from deepmimic_mujoco_amd.vec_env import HipBatchEnv

N = 6
SHAPES = {"dpenv": (67, 5, 28, LazyInfos), "combined": (98, 8, 23, _LazyCombinedInfos)}


class FakeEngine:
    def __init__(self, nk, k, obs_dim, terms_dim):
        self.N, self.k, self.obs_dim, self.terms_dim = nk, k, obs_dim, terms_dim
        self.device, self.calls, self.n_steps = torch.device("cpu"), [], 0

    def expected(self, step):
        """The six outputs of this engine's rows at step number ``step`` (float64 / int numpy)."""
        g = np.arange(self.N) + self.k * self.N                           # global env index
        obs = g[:, None] * 100.0 + step + np.arange(self.obs_dim)[None] / 256.0
        return dict(obs=obs, rew=g + step / 16.0, done=(g + step) % 2, terms=g[:, None] * 10.0 + np.arange(self.terms_dim)[None] + step / 4.0,
                    reason=(g + step) % 8, terminal_obs=-obs)

    def step(self, actions, out):
        self.n_steps += 1
        self.calls.append(("step", actions))
        for name, v in self.expected(self.n_steps).items():
            out[name].copy_(torch.as_tensor(v).to(out[name].dtype))

    def reset(self, obs, idx_init=None, mask=None):
        self.calls.append(("reset", idx_init))
        obs.fill_(float(self.k))

    def set_seed(self, seed):
        self.calls.append(("set_seed", seed))

    def close(self):
        self.calls.append(("close",))


def _model(n_actions):
    return types.SimpleNamespace(act_ctrlrange=np.stack([-np.arange(1.0, n_actions + 1), np.arange(1.0, n_actions + 1)], 1),
                                 body_parent=np.zeros(3, np.int32))


def _build(self, shape, sub_batches):
    d, k, a, infos = SHAPES[shape]
    HipBatchEnv.__init__(self, N, sub_batches, lambda nk, i: FakeEngine(nk, i, d, k), _model(a), d, k, a, infos=infos)


class SerialEnv(HipBatchEnv):            # the base joins its engines in order on the current stream (the humanoid classes)
    __init__ = _build


class ForkJoinEnv(g1.HipG1VecEnv):       # the G1 classes' override; a sibling constructor keeps the real engines out
    __init__ = _build


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sub_batches", [1, 3])
def test_step_wait_returns_exactly_what_the_engines_wrote(shape, sub_batches):
    d, k, a, infos_cls = SHAPES[shape]
    env = SerialEnv(shape, sub_batches)
    assert env.observation_space.shape == (d,) and env.action_space.shape == (a,) and env._actions.shape == (N, a)
    assert env.render_mode is None and env.reset_infos == [{}] * N and env.engine is env.engines[0]
    assert np.array_equal(env.reset(), np.repeat(np.arange(sub_batches), N // sub_batches)[:, None] * np.ones((1, d)))
    for step in (1, 2):
        obs, rew, done, infos = env.step(np.zeros((N, a)))
        want = {name: np.concatenate([e.expected(step)[name] for e in env.engines]) for name in env.out}
        assert obs.dtype == np.float32 and np.array_equal(obs, want["obs"]) and np.array_equal(rew, want["rew"])
        assert done.dtype == bool and np.array_equal(done, want["done"] != 0)
        assert type(infos) is infos_cls and len(infos) == N
        make = _combined_info if k == 8 else _make_info
        for i, info in enumerate(infos):
            assert ("terminal_observation" in info) == bool(done[i])
            if done[i]:
                assert np.array_equal(info.pop("terminal_observation"), want["terminal_obs"][i])
            assert info == make(want["terms"][i].astype(np.float32), int(want["reason"][i]))
            assert info.get("done_reason") == (None if want["reason"][i] in (5, 6) else _lib.REASONS.get(int(want["reason"][i])))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sub_batches_are_views_and_each_engine_steps_its_rows_once_in_order(shape):
    env = SerialEnv(shape, 3)
    assert env.sub_slices == [slice(0, 2), slice(2, 4), slice(4, 6)] and len(env.engines) == 3
    for k, sl in enumerate(env.sub_slices):
        for name, v in env.out.items():
            assert env.sub_out[k][name].data_ptr() == v[sl].data_ptr() and env.sub_out[k][name].shape == v[sl].shape, (k, name)
    order = []
    for e in env.engines:
        e.calls = order                                                    # one shared log shows the order across engines
    actions = torch.arange(N * env._actions.shape[1], dtype=torch.float32).reshape(env._actions.shape)
    assert env.step_tensor(actions) is env.out
    assert [c[0] for c in order] == ["step"] * 3
    for k, (_, rows) in enumerate(order):
        assert torch.equal(rows, actions[env.sub_slices[k]])
    assert [e.n_steps for e in env.engines] == [1, 1, 1]
    before = {name: v.clone() for name, v in env.out.items()}
    assert env.step_sub(1, actions[2:4]) is env.sub_out[1]
    assert [e.n_steps for e in env.engines] == [1, 2, 1]
    for name, v in env.out.items():
        assert torch.equal(v[0:2], before[name][0:2]) and torch.equal(v[4:6], before[name][4:6]), name
    assert not torch.equal(env.out["obs"][2:4], before["obs"][2:4])


@pytest.mark.parametrize("cls", [SerialEnv, ForkJoinEnv])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_engine_gets_one_step_call_with_the_callers_tensor(cls, shape):
    env = cls(shape, 1)                  # the fork/join class runs with one sub-batch only: a CPU has no streams
    assert env.sub_out[0] is env.out
    actions = torch.ones(env._actions.shape)
    env.step_tensor(actions)
    (name, got), = env.engine.calls
    assert name == "step" and got is actions


def test_seed_keys_engine_k_with_seed_plus_104729_k():
    env = SerialEnv("dpenv", 3)
    assert env.seed(7) == [7, 8, 9, 10, 11, 12]
    assert [e.calls for e in env.engines] == [[("set_seed", 7 + 104729 * k)] for k in range(3)]
    assert env.seed(None) == [None] * 6 and all(len(e.calls) == 1 for e in env.engines)


def test_protocol_methods_honour_indices_and_close_every_engine():
    env = SerialEnv("combined", 3)
    with pytest.raises(AttributeError):
        env.env_method("no_such_method")
    assert env.get_attr("num_envs") == [6] * 6 and env.get_attr("num_envs", indices=[0, 3]) == [6, 6]
    assert env.env_is_wrapped(object) == [False] * 6 and env.env_is_wrapped(object, indices=4) == [False]
    assert env.env_method("seed", 5, indices=[1, 2]) == [[5, 6, 7, 8, 9, 10]] * 2
    env.set_attr("marker", 3, indices=[0])
    assert env.get_attr("marker", indices=[5]) == [3] and env.unwrapped is env and env.getattr_depth_check("x", False) is None
    env.close()
    assert all(e.calls[-1] == ("close",) for e in env.engines)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_async_takes_c_fortran_and_flat_float64_actions(shape):
    env = SerialEnv(shape, 1)
    a = np.random.default_rng(0).uniform(-1, 1, env._actions.shape)
    want = torch.tensor(a.astype(np.float32))
    for given in (np.ascontiguousarray(a), np.asfortranarray(a), a.reshape(-1)):
        env._actions.zero_()
        env.step_async(given)
        assert torch.equal(env._actions, want) and env._actions.is_contiguous()


TERMS = np.array([0.5, 0.25, 0.125, 2.0, 4.0, 8.0, 16.0, 3.0], np.float32)
HAND_BUILT = {"reward_config": 0.5, "reward_qvel": 0.25, "reward_end_eff": 0.125, "reward_com": 2.0, "reward_joint_limit": 4.0,
              "imitation_reward": 8.0, "task_reward": 16.0}       # what G1CombinedEnv.step used to spell out key by key


@pytest.mark.parametrize("reason,want", [(0, HAND_BUILT), (3, dict(HAND_BUILT, done_reason="max_ep_len")),
                                         (7, dict(HAND_BUILT, done_reason="fallen without amnesty")), (5, {}), (6, {}),
                                         (8, dict(HAND_BUILT, done_reason="run roll/pitch limit"))])
def test_combined_info_is_the_dict_g1combinedenv_built_by_hand(reason, want):
    got = _combined_info(TERMS, reason, g1.REASONS)
    assert got == want and all(type(v) is (str if k == "done_reason" else float) for k, v in got.items())
    if reason != 8:                                                       # the humanoid table stops at 7
        assert _combined_info(TERMS, reason) == want


def test_make_info_names_the_reason_from_the_table_it_is_given():
    five = {k: v for k, v in HAND_BUILT.items() if k.startswith("reward_")}
    assert _make_info(TERMS[:5], 8, g1.REASONS) == dict(five, done_reason="run roll/pitch limit")
    assert _make_info(TERMS[:5], 8) == five and _make_info(TERMS[:5], 1) == dict(five, done_reason="low_z")
    assert _make_info(TERMS[:5], 5, g1.REASONS) == {} and _make_info(TERMS[:5], 6) == {}
