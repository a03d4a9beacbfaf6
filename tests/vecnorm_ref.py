"""SB3's ``RunningMeanStd`` and ``VecNormalize`` [EXT] restated in numpy fp64: the oracle of the vec-normalize tests.  Nothing else."""
import numpy as np


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.update_from_moments(x.mean(axis=0), x.var(axis=0), x.shape[0])

    def update_from_moments(self, bm, bv, n):
        d = bm - self.mean
        tot = self.count + n
        self.mean = self.mean + d * n / tot
        self.var = (self.var * self.count + bv * n + np.square(d) * self.count * n / tot) / tot
        self.count = tot


class VecNormalizeRef:
    """The wrapper's arithmetic on what the inner env returned (the env itself is the caller's)."""

    def __init__(self, num_envs, obs_dim, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99,
                 epsilon=1e-8):
        self.obs_rms, self.ret_rms = RunningMeanStd((obs_dim,)), RunningMeanStd(())
        self.returns = np.zeros(num_envs, np.float64)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon

    def normalize_obs(self, x):
        if not self.norm_obs:
            return np.asarray(x, np.float32)
        y = (np.asarray(x, np.float64) - self.obs_rms.mean) / np.sqrt(self.obs_rms.var + self.epsilon)
        return np.clip(y, -self.clip_obs, self.clip_obs).astype(np.float32)

    def normalize_reward(self, r):
        if not self.norm_reward:
            return np.asarray(r, np.float32)
        y = np.asarray(r, np.float64) / np.sqrt(self.ret_rms.var + self.epsilon)
        return np.clip(y, -self.clip_reward, self.clip_reward).astype(np.float32)

    def reset(self, obs):
        self.returns[:] = 0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs)

    def step(self, obs, rew, done, tobs=None):
        """-> (obs, rew, tobs) normalised; tobs rows of envs that are not done come back unchanged."""
        done = np.asarray(done) != 0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        new_obs = self.normalize_obs(obs)
        if self.training:
            self.returns = self.returns * self.gamma + np.asarray(rew, np.float64)
            self.ret_rms.update(self.returns)
        new_rew = self.normalize_reward(rew)
        new_tobs = None
        if tobs is not None:
            new_tobs = np.asarray(tobs, np.float32).copy()
            new_tobs[done] = self.normalize_obs(np.asarray(tobs)[done])
        self.returns[done] = 0
        return new_obs, new_rew, new_tobs
