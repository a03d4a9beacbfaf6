"""Reference of the rollout monitor, written without the project (not a conftest, not a test): SB3's Monitor + ``ep_info_buffer``
for a vec-env fed with [T, N] reward / done arrays, and SB3's ``explained_variance`` in fp64.

Per env a running episode return (fp32, summed in step order) and length; a finished episode goes into a
``collections.deque(maxlen=100)`` in the order SB3's ``_update_info_buffer`` meets them: rollout by rollout, step by step, env by
env.  Returns are not rounded to six decimals (SB3's Monitor does that for its csv)."""
import collections

import numpy as np

HIST = 100


class MonitorRef:
    def __init__(self, n_envs):
        self.ret = [np.float32(0.0)] * n_envs
        self.len = [0] * n_envs
        self.buffer = collections.deque(maxlen=HIST)        # (return, length), oldest first
        self.episodes = 0

    def feed(self, rew, done):
        """One rollout: rew [T, N] fp32, done [T, N] (anything non-zero ends the episode at that step)."""
        rew = np.asarray(rew, dtype=np.float32)
        done = np.asarray(done)
        T, N = rew.shape
        for t in range(T):
            for e in range(N):
                self.ret[e] = np.float32(self.ret[e] + rew[t, e])
                self.len[e] += 1
                if done[t, e] != 0:
                    self.buffer.append((self.ret[e], self.len[e]))
                    self.episodes += 1
                    self.ret[e] = np.float32(0.0)
                    self.len[e] = 0

    def returns(self):
        return np.array([r for r, _ in self.buffer], dtype=np.float32)

    def lengths(self):
        return np.array([l for _, l in self.buffer], dtype=np.float32)

    def slots(self):
        """The history as a ring of 100 slots, episode m in slot m mod 100 (zeros where nothing was written): [2, 100] fp32."""
        out = np.zeros((2, HIST), dtype=np.float32)
        first = self.episodes - len(self.buffer)
        for i, (r, l) in enumerate(self.buffer):
            out[0, (first + i) % HIST], out[1, (first + i) % HIST] = r, l
        return out

    def running(self):
        """[2, N] fp32: return | length of every env's unfinished episode."""
        return np.stack([np.array(self.ret, dtype=np.float32), np.array(self.len, dtype=np.float32)])

    @property
    def ep_rew_mean(self):
        return float(np.mean(self.returns().astype(np.float64))) if self.buffer else float("nan")

    @property
    def ep_len_mean(self):
        return float(np.mean(self.lengths().astype(np.float64))) if self.buffer else float("nan")


def explained_variance(values, returns):
    """SB3: 1 - Var[y_true - y_pred] / Var[y_true] over the flattened buffer, population variances, NaN when Var[y_true] = 0; fp64."""
    y = np.asarray(returns, dtype=np.float64).reshape(-1)
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    vy = np.var(y)
    return float("nan") if vy == 0 else float(1.0 - np.var(y - v) / vy)


def same(a, b):
    """Equal floats, NaN equal to NaN."""
    return (a != a and b != b) or a == b
