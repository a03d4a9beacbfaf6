"""``HipVecNormalize(sync_group=...)`` restated in numpy fp64 for W simulated ranks: per rank ``base`` (what all ranks
agreed on at the last synchronisation), ``acc`` (what the rank alone has seen since, empty = count 0) and ``running`` =
merge(base, acc), every merge being ``update_from_moments`` of tests/vecnorm_ref.py with a set of count 0 skipped exactly.
The oracle of the synchronised vec-normalize tests.  Nothing else."""
import numpy as np

from vecnorm_ref import RunningMeanStd, VecNormalizeRef


def merge(a, b):
    """merge(a, b) of two (mean, var, count) triples -> a new triple; b is the batch of ``update_from_moments``."""
    if b[2] == 0:
        return a
    if a[2] == 0:
        return b
    r = RunningMeanStd(np.shape(a[0]))
    r.mean, r.var, r.count = np.asarray(a[0], np.float64), np.asarray(a[1], np.float64), float(a[2])
    r.update_from_moments(np.asarray(b[0], np.float64), np.asarray(b[1], np.float64), float(b[2]))
    return (r.mean, r.var, r.count)


def batch_moments(x):
    x = np.asarray(x, np.float64)
    return (x.mean(axis=0), x.var(axis=0), float(x.shape[0]))


def empty(shape):
    return (np.zeros(shape, np.float64), np.zeros(shape, np.float64), 0.0)


def start(shape):
    return (np.zeros(shape, np.float64), np.ones(shape, np.float64), 1e-4)


def flat(obs, ret):
    """The [2 D + 4] layout of ``HipVecNormalize._state``: obs mean | obs var | obs count | ret mean, var, count."""
    return np.concatenate([obs[0], obs[1], [obs[2]], [float(ret[0])], [float(ret[1])], [ret[2]]]).astype(np.float64)


def unflat(row, D):
    row = np.asarray(row, np.float64)
    return (row[:D].copy(), row[D:2 * D].copy(), float(row[2 * D])), (np.float64(row[2 * D + 1]), np.float64(row[2 * D + 2]), float(row[2 * D + 3]))


class SyncRankRef(VecNormalizeRef):
    """One rank: ``VecNormalizeRef`` whose two ``RunningMeanStd`` hold ``running`` and are rebuilt from base and acc on every update."""

    def __init__(self, num_envs, obs_dim, **kw):
        super().__init__(num_envs, obs_dim, **kw)
        self.D = obs_dim
        self.base = [start((obs_dim,)), start(())]
        self.acc = [empty((obs_dim,)), empty(())]
        for k, rms in enumerate((self.obs_rms, self.ret_rms)):
            rms.update = lambda x, k=k: self._update(k, x)

    def _update(self, k, x):
        self.acc[k] = merge(self.acc[k], batch_moments(x))
        self._set_running(k, merge(self.base[k], self.acc[k]))

    def _set_running(self, k, m):
        rms = (self.obs_rms, self.ret_rms)[k]
        rms.mean, rms.var, rms.count = m

    def acc_row(self):
        return flat(*self.acc)

    def base_row(self):
        return flat(*self.base)

    def running_row(self):
        return flat((self.obs_rms.mean, self.obs_rms.var, self.obs_rms.count), (self.ret_rms.mean, self.ret_rms.var, self.ret_rms.count))

    def merge_rows(self, rows):
        """The merge launch: base = merge(base, row 0, row 1, ...), acc emptied, running = base."""
        for row in rows:
            for k, m in enumerate(unflat(row, self.D)):
                self.base[k] = merge(self.base[k], m)
        self.acc = [empty((self.D,)), empty(())]
        for k in (0, 1):
            self._set_running(k, self.base[k])


def sync(ranks):
    """``sync()`` on every rank of the group: each sees every rank's acc, in rank order."""
    rows = [r.acc_row() for r in ranks]
    for r in ranks:
        r.merge_rows(rows)
