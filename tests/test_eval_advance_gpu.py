"""``dm_eval_advance`` (csrc/dm_eval.hip) on the GPU against a numpy restatement of its contract: per-step exact equality of the
episode bookkeeping, of the compacted list of live envs and of the fp64 sums (bit for bit), at sizes around the wave (64) and chunk
(1 024) boundaries; stale rows of finished envs are poisoned and must not be read; guard words behind every output stay intact."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _lib

pytestmark = pytest.mark.gpu

TERMS, OBS, STEPS, G = 5, 67, 12, 16
TRUNCATED = -1


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Arrays:
    """Device-side state of one evaluation, every output array between two rows of G guard elements."""

    SPEC = dict(alive=(torch.uint8, 1, 0xA5), ep_len=(torch.int32, 1, -777), ep_ret=(torch.float64, 1, -1.5e300),
                ep_terms=(torch.float64, TERMS, -2.5e300), ep_reason=(torch.int32, 1, -778), last_obs=(torch.float32, OBS, -3.5e30),
                env_ids=(torch.int32, 1, -779), count=(torch.int32, 1, -780))

    def __init__(self, n, dev):
        self.n, self.full, self.v = n, {}, {}
        for name, (dt, w, guard) in self.SPEC.items():
            rows = 1 if name == "count" else n
            full = torch.full((G + rows * w + G,), guard, dtype=dt, device=dev)
            full[G:G + rows * w] = 0
            self.full[name] = full
            self.v[name] = full[G:G + rows * w].view(rows, w) if w > 1 else full[G:G + rows * w]
        self.v["alive"].fill_(1)
        self.v["env_ids"].copy_(torch.arange(n, dtype=torch.int32, device=dev))

    def guards_intact(self):
        for name, (dt, w, guard) in self.SPEC.items():
            f = self.full[name]
            g = torch.full((G,), guard, dtype=dt, device=f.device)
            if not (torch.equal(f[:G], g) and torch.equal(f[-G:], g)):
                return name
        return None

    def host(self):
        return {k: v.cpu().numpy().copy() for k, v in self.v.items()}


def advance(L, A, n, max_steps, rew, done, reason, terms, obs, dev):
    v = A.v
    return L.dm_eval_advance(n, TERMS, max_steps, _p(rew), _p(done), _p(reason), _p(terms), _p(obs), OBS, _p(v["alive"]), _p(v["ep_len"]),
                             _p(v["ep_ret"]), _p(v["ep_terms"]), _p(v["ep_reason"]), _p(v["last_obs"]), _p(v["env_ids"]), _p(v["count"]),
                             dev.index or 0, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))


def numpy_advance(S, max_steps, rew, done, reason, terms, obs):
    """The contract of include/deepmimic_hip.h, restated: S holds alive, ep_len, ep_ret, ep_terms, ep_reason, last_obs."""
    m = S["alive"] != 0
    S["ep_len"][m] += 1
    S["ep_ret"][m] += rew[m].astype(np.float64)
    S["ep_terms"][m] += terms[m].astype(np.float64)
    d = m & (done != 0)
    cut = m & ~d & (S["ep_len"] == max_steps)
    S["ep_reason"][d] = reason[d]
    S["ep_reason"][cut] = TRUNCATED
    fin = d | cut
    S["last_obs"][fin] = obs[fin]
    S["alive"][fin] = 0
    live = np.nonzero(S["alive"])[0].astype(np.int32)
    S["env_ids"] = np.concatenate([live, np.full(len(m) - len(live), -1, np.int32)])
    S["count"] = np.array([len(live)], np.int32)


def done_stream(pattern, n, rng):
    """[STEPS, n] done flags and max_steps of a pattern."""
    d = np.zeros((STEPS, n), np.uint8)
    max_steps = 100
    if pattern == "nobody":
        pass
    elif pattern == "everybody_on_step_1":
        d[0] = 1
    elif pattern == "alternate":
        d[2, 0::2] = 1
        d[7, 1::4] = 1
    elif pattern == "only_the_last":
        d[1, n - 1] = 1
    elif pattern == "cap_with_done":                      # max_steps falls on step 5; a third of the envs is done on that very step
        max_steps = 5
        d[4, 0::3] = 1
        d[1, 1::7] = 1
    elif pattern == "random":
        d = (rng.random((STEPS, n)) < 0.15).astype(np.uint8)
        max_steps = 9
    return d, max_steps


PATTERNS = ["nobody", "everybody_on_step_1", "alternate", "only_the_last", "cap_with_done", "random"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 2500])
def test_eval_advance_matches_the_numpy_restatement(n):
    dev = torch.device("cuda", 0)
    L = _lib.load_library()
    up = lambda a: torch.as_tensor(a, device=dev).contiguous()
    for pi, pattern in enumerate(PATTERNS):
        rng = np.random.default_rng(1000 * n + pi)
        dones, max_steps = done_stream(pattern, n, rng)
        A = Arrays(n, dev)
        S = A.host()
        finished_any = False
        for t in range(STEPS):
            rew = rng.standard_normal(n).astype(np.float32)
            reason = rng.integers(1, 8, n).astype(np.int32)
            terms = rng.standard_normal((n, TERMS)).astype(np.float32)
            obs = rng.standard_normal((n, OBS)).astype(np.float32)
            done = dones[t].copy()
            dead = S["alive"] == 0                         # rows of envs that finished earlier are stale: poison them
            rew[dead], done[dead], reason[dead], terms[dead], obs[dead] = np.nan, 1, 99, np.nan, np.nan
            finished_any |= bool(dead.any())
            rc = advance(L, A, n, max_steps, up(rew), up(done), up(reason), up(terms), up(obs), dev)
            assert rc == 0
            numpy_advance(S, max_steps, rew, done, reason, terms, obs)
            got = A.host()
            where = "%s, n %d, step %d" % (pattern, n, t + 1)
            for k in ("alive", "ep_len", "ep_reason", "env_ids", "count"):
                assert np.array_equal(got[k], S[k]), (where, k)
            assert np.array_equal(got["ep_ret"].view(np.int64), S["ep_ret"].view(np.int64)), where          # bit for bit
            assert np.array_equal(got["ep_terms"].view(np.int64), S["ep_terms"].view(np.int64)), where
            assert np.array_equal(got["last_obs"].view(np.int32), S["last_obs"].view(np.int32)), where
            ids, c = got["env_ids"], int(got["count"][0])
            assert np.all(np.diff(ids[:c]) > 0) and np.all(ids[c:] == -1)                                   # ascending, -1 tail
            assert A.guards_intact() is None, (where, A.guards_intact())
        if pattern == "nobody":
            assert int(S["count"][0]) == n and np.all(S["ep_len"] == STEPS)
        if pattern in ("everybody_on_step_1", "cap_with_done", "random"):
            assert int(S["count"][0]) == 0 and finished_any
            # with nobody alive a call changes nothing, whatever the (stale) inputs hold
            before = A.host()
            nan = torch.full((n,), float("nan"), device=dev)
            rc = advance(L, A, n, max_steps, nan, torch.ones(n, dtype=torch.uint8, device=dev), torch.full((n,), 99, dtype=torch.int32, device=dev),
                         torch.full((n, TERMS), float("nan"), device=dev), torch.full((n, OBS), float("nan"), device=dev), dev)
            assert rc == 0
            after = A.host()
            for k in before:
                assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (pattern, n, k)
            assert A.guards_intact() is None
        if pattern == "cap_with_done":
            assert np.all(S["ep_reason"][0::3][S["ep_len"][0::3] == 5] != TRUNCATED)                         # done wins on the cap step
            assert np.any(S["ep_reason"] == TRUNCATED) or n < 3


def test_eval_advance_without_the_optional_arrays_and_bad_arguments():
    dev = torch.device("cuda", 0)
    L = _lib.load_library()
    n = 130
    A = Arrays(n, dev)
    v = A.v
    rew = torch.arange(n, dtype=torch.float32, device=dev)
    done = (torch.arange(n, device=dev) % 3 == 0).to(torch.uint8)
    reason = torch.full((n,), 2, dtype=torch.int32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    # terms, obs and last_obs are optional
    rc = L.dm_eval_advance(n, 0, 10, _p(rew), _p(done), _p(reason), None, None, 0, _p(v["alive"]), _p(v["ep_len"]), _p(v["ep_ret"]), None,
                           _p(v["ep_reason"]), None, _p(v["env_ids"]), _p(v["count"]), 0, s)
    assert rc == 0
    got = A.host()
    live = np.nonzero(np.arange(n) % 3 != 0)[0]
    assert int(got["count"][0]) == len(live) and np.array_equal(got["env_ids"][:len(live)], live)
    assert np.array_equal(got["ep_ret"], np.arange(n, dtype=np.float64)) and not got["ep_terms"].any() and not got["last_obs"].any()
    assert A.guards_intact() is None
    # refusals: nothing is launched
    bad = [dict(n=0), dict(max_steps=0), dict(rew=None), dict(done=None), dict(reason=None), dict(alive=None), dict(env_ids=None),
           dict(count=None), dict(device=-1)]
    for b in bad:
        a = dict(n=n, max_steps=10, rew=_p(rew), done=_p(done), reason=_p(reason), alive=_p(v["alive"]), env_ids=_p(v["env_ids"]),
                 count=_p(v["count"]), device=0)
        a.update(b)
        rc = L.dm_eval_advance(a["n"], 0, a["max_steps"], a["rew"], a["done"], a["reason"], None, None, 0, a["alive"], _p(v["ep_len"]),
                               _p(v["ep_ret"]), None, _p(v["ep_reason"]), None, a["env_ids"], a["count"], a["device"], s)
        assert rc == -22, b
    terms = torch.zeros(n, TERMS, device=dev)
    rc = L.dm_eval_advance(n, TERMS, 10, _p(rew), _p(done), _p(reason), _p(terms), None, 0, _p(v["alive"]), _p(v["ep_len"]), _p(v["ep_ret"]),
                           None, _p(v["ep_reason"]), None, _p(v["env_ids"]), _p(v["count"]), 0, s)
    assert rc == -22                                        # terms without ep_terms
    torch.cuda.synchronize()
    after = A.host()
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), after[k].view(np.uint8)), k
