"""The episode debug log's ring, mark, trigger and slot rules in numpy, restated from their specification (no project code).

Per env a ring of K rows of W = nq + 2 nv + na + 5 float32: qpos | qvel | qacc_warmstart | action | reward, done, reason, kind,
step, the last four as int32 bit patterns.  Entry j of an env (j counts that env's entries from 0) lives in row j mod K and stores
step = j.  kind 0 is a step (state after it, action given to it, what it returned), kind 1 a mark (a state set from outside; zero
action, reward, done, reason).  ``head[env]`` counts the entries ever written.

After the entries of one ``record`` call are written, every listed env with done != 0 and bit ``reason`` set in ``reason_mask`` is a
trigger.  The triggers of one call take the next free slots of ``cap`` in ascending env order; a filed slot receives that env's ring
oldest entry first, min(head, K) rows, and ``cap_meta`` = {env, valid entries, head at the trigger, reason}.  ``cap_count`` =
{copies filed (at most C), triggers seen}; triggers beyond C are only counted.  Rows and slots never written stay zero.  A listed
env outside [0, N) is skipped.
"""
import numpy as np


def _i2f(x):
    return np.array([x], np.int32).view(np.float32)[0]


class TraceRef:
    def __init__(self, N, K, C, nq, nv, na, reason_mask):
        self.N, self.K, self.C, self.nq, self.nv, self.na = N, K, C, nq, nv, na
        self.W = nq + 2 * nv + na + 5
        self.mask = int(reason_mask)
        self.ring = np.zeros((N, K, self.W), np.float32)
        self.head = np.zeros(N, np.int64)
        self.cap = np.zeros((C, K, self.W), np.float32)
        self.cap_meta = np.zeros((C, 4), np.int32)
        self.cap_count = np.zeros(2, np.int32)

    def _listed(self, env_ids, nslots):
        ids = range(self.N) if env_ids is None else [int(e) for e in np.asarray(env_ids)[:nslots]]
        return [e for e in ids if 0 <= e < self.N]

    def _entry(self, env, qpos, qvel, warm, action, reward, done, reason, kind):
        row = np.zeros(self.W, np.float32)
        o1, o2, o3, o4 = self.nq, self.nq + self.nv, self.nq + 2 * self.nv, self.nq + 2 * self.nv + self.na
        row[:o1], row[o1:o2], row[o2:o3] = qpos, qvel, warm
        row[o3:o4] = action
        row[o4] = reward
        row[o4 + 1], row[o4 + 2], row[o4 + 3], row[o4 + 4] = _i2f(done), _i2f(reason), _i2f(kind), _i2f(int(self.head[env]))
        self.ring[env, self.head[env] % self.K] = row
        self.head[env] += 1

    def ordered(self, env):
        """The env's ring oldest entry first: [min(head, K), W]."""
        h = int(self.head[env])
        n = min(h, self.K)
        return self.ring[env, [(h - n + r) % self.K for r in range(n)]]

    def mark(self, qpos, qvel, warm, env_ids=None, nslots=None):
        for e in self._listed(env_ids, nslots):
            self._entry(e, qpos[e], qvel[e], warm[e], 0.0, 0.0, 0, 0, 1)

    def record(self, qpos, qvel, warm, actions, rew, done, reason, env_ids=None, nslots=None):
        listed = self._listed(env_ids, nslots)
        for e in listed:
            self._entry(e, qpos[e], qvel[e], warm[e], actions[e], rew[e], int(done[e] != 0), int(reason[e]), 0)
        for e in sorted(listed):
            if done[e] != 0 and 0 <= int(reason[e]) < 32 and (self.mask >> int(reason[e])) & 1:
                slot = int(self.cap_count[0])
                if slot < self.C:
                    rows = self.ordered(e)
                    self.cap[slot, :len(rows)] = rows
                    self.cap_meta[slot] = [e, len(rows), int(self.head[e]), int(reason[e])]
                    self.cap_count[0] += 1
                self.cap_count[1] += 1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)
