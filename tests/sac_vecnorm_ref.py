"""SB3's SAC on a ``VecNormalize`` env [EXT: OffPolicyAlgorithm.collect_rollouts / _store_transition, ReplayBuffer._get_samples]
restated in numpy fp64 on top of tests/vecnorm_ref.py, and the envs of the SAC + VecNormalize tests.  Not a conftest.

The sequence, per vec-env step:
  1. the action comes from the actor on ``obs_norm`` (the caller's business: the reference hands out ``obs_norm``);
  2. the inner env steps: raw ``obs``, ``rew``, ``done``, ``terminal_obs``;
  3. ``VecNormalize.step_wait``: obs_rms.update(obs), returns / ret_rms update (when training, warm-up included);
  4. the ring gets the RAW last observation, the action in [-1, 1], the raw reward, done, and as next observation the raw new
     observation, or the raw terminal observation of a finished env;
  5. a minibatch of rows ``idx`` is normalize_obs(obs), act, normalize_reward(rew), normalize_obs(next_obs), done, with the
     statistics of the moment of the sample; nothing is updated.
One stated deviation from SB3, DESIGN §7: SB3 stores unnormalize_obs(normalize_obs(terminal_obs)), which differs from the raw terminal
observation in columns clipped at store time and by one fp32 rounding; here the ring holds the raw one."""
import numpy as np
import torch

from sac_helpers import BanditEnv
from vecnorm_ref import VecNormalizeRef


class SacVecNormRef:
    def __init__(self, n, D, A, cap_steps, **vn_kw):
        self.n, self.cap = n, cap_steps
        self.vn = VecNormalizeRef(n, D, **vn_kw)
        rows = n * cap_steps
        self.ring = dict(obs=np.zeros((rows, D), np.float32), act=np.zeros((rows, A), np.float32), rew=np.zeros(rows, np.float32),
                         done=np.zeros(rows, np.float32), next_obs=np.zeros((rows, D), np.float32))
        self.pos = self.fill = 0
        self.last_raw = self.obs_norm = None

    def reset(self, obs):
        self.last_raw = np.array(obs, np.float32)
        self.obs_norm = self.vn.reset(obs)
        return self.obs_norm

    def step(self, act, obs, rew, done, terminal_obs):
        """``act`` in [-1, 1] is what was taken on ``obs_norm``; the rest is what the inner env returned."""
        d = np.asarray(done) != 0
        new_norm, _, _ = self.vn.step(obs, rew, done)
        sl = slice(self.pos * self.n, (self.pos + 1) * self.n)
        R = self.ring
        R["obs"][sl], R["act"][sl], R["rew"][sl], R["done"][sl] = self.last_raw, act, rew, d
        R["next_obs"][sl] = np.where(d[:, None], terminal_obs, obs)
        self.pos, self.fill = (self.pos + 1) % self.cap, min(self.fill + 1, self.cap)
        self.last_raw, self.obs_norm = np.array(obs, np.float32), new_norm
        return new_norm

    def sample(self, idx):
        R, vn = self.ring, self.vn
        return dict(obs=vn.normalize_obs(R["obs"][idx]), act=R["act"][idx], rew=vn.normalize_reward(R["rew"][idx]),
                    next_obs=vn.normalize_obs(R["next_obs"][idx]), done=R["done"][idx])


def normalize_batch64(vn, batch):
    """The fp64 minibatch a fp64 learner reads: ``vn`` (a VecNormalizeRef) applied to raw ring rows WITHOUT the final cast to fp32."""
    def obs(x):
        y = (np.asarray(x, np.float64) - vn.obs_rms.mean) / np.sqrt(vn.obs_rms.var + vn.epsilon)
        return np.clip(y, -vn.clip_obs, vn.clip_obs) if vn.norm_obs else np.asarray(x, np.float64)
    rew = np.asarray(batch["rew"], np.float64)
    if vn.norm_reward:
        rew = np.clip(rew / np.sqrt(vn.ret_rms.var + vn.epsilon), -vn.clip_reward, vn.clip_reward)
    return dict(obs=obs(batch["obs"]), act=np.asarray(batch["act"], np.float64), rew=rew, next_obs=obs(batch["next_obs"]),
                done=np.asarray(batch["done"], np.float64))


def out_bound(ref):
    """The project's bound on a normalised output: one rounding to fp32 plus fp64 reordering noise."""
    return 2.0 ** -23 * np.abs(np.asarray(ref, np.float64)) + 1e-9


def stats_of(vn):
    """(obs mean, obs var, obs count, ret mean, ret var, ret count) of a HipVecNormalize as numpy fp64."""
    return (vn.obs_rms.mean, vn.obs_rms.var, np.array([vn.obs_rms.count]), vn.ret_rms.mean.reshape(-1), vn.ret_rms.var.reshape(-1),
            np.array([vn.ret_rms.count]))


def ref_stats_of(ref):
    return (ref.obs_rms.mean, ref.obs_rms.var, np.array([ref.obs_rms.count]), np.array([ref.ret_rms.mean]), np.array([ref.ret_rms.var]),
            np.array([ref.ret_rms.count]))


def stats_rel_err(vn, ref):
    """Worst relative error of the six statistics (absolute where the reference is 0)."""
    worst = 0.0
    for got, want in zip(stats_of(vn), ref_stats_of(ref)):
        want = np.asarray(want, np.float64)
        worst = max(worst, float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.where(want == 0, 1.0, np.abs(want)))))
    return worst


class RecordingBandit(BanditEnv):
    """BanditEnv that keeps copies of what it returned: ``first`` (reset) and ``log`` (one dict per step, the action included)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.first, self.log = None, []

    def reset_tensor(self):
        obs = super().reset_tensor()
        self.first = obs.clone()
        return obs

    def step_tensor(self, actions):
        out = super().step_tensor(actions)
        self.log.append(dict({k: v.clone() for k, v in out.items()}, act_env=actions.clone()))
        return out


class ScaledBanditEnv(BanditEnv):
    """The same bandit behind badly scaled sensors: the first half of the observation columns is presented as 50 + 1e-3 x (a large
    mean, a small spread), the second half as 1e3 x.  Rewards and the optimum are those of the underlying x."""

    def present(self, x):
        h = self.D // 2
        return torch.cat([50.0 + 1e-3 * x[:, :h], 1e3 * x[:, h:]], 1).contiguous()

    def reset_tensor(self):
        return self.present(super().reset_tensor())

    def step_tensor(self, actions):
        out = super().step_tensor(actions)
        out["obs"], out["terminal_obs"] = self.present(out["obs"]), self.present(out["terminal_obs"])
        return out
