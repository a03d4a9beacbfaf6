"""SAC's n-step minibatch (include/deepmimic_sac_nstep.h; SB3 >= 2.7 NStepReplayBuffer) restated in numpy fp64, one row at a time,
and the rings of the n-step tests.  Not a conftest.

Ring: row(s, e) = s * N + e over ``cap`` steps, ``pos`` the write position, ``fill`` the stored steps, newest = (pos + cap - 1) mod cap.
Minibatch row of ring row i = (t, e): walk s_j = (t + j) mod cap for j = 0 .. n - 1 and stop AFTER the first j with done(s_j, e) = 1,
s_j = newest, or j = n - 1; k = j + 1, last = row(s_(k-1), e); obs and act of row i, next_obs of row last, rew = sum_{j<k} gamma^j r_j,
done' = 1 - gamma^(k-1) (1 - done(last)).  gamma is the fp32 value the kernels receive.  With a normaliser (a VecNormalizeRef) every
r_j goes through normalize_reward on its own before it is discounted and obs / next_obs through normalize_obs, all in fp64 without
the cast to fp32 (normalize_batch64 of tests/sac_vecnorm_ref.py)."""
import numpy as np

from sac_vecnorm_ref import normalize_batch64, out_bound

U = 2.0 ** -24                   # half an ulp of 1 in fp32


def nstep_batch64(ring, idx, N, cap, pos, n, gamma, vn=None):
    """-> dict of fp64 arrays obs, act, rew, next_obs, done (= done'), and k, last (int), S = sum_{j<k} gamma^j |r_j| and
    rew_norm_bound = sum_{j<k} gamma^j out_bound(r_j) (0 without a normaliser), kinds (a set of strings per row, for coverage)."""
    g = float(np.float32(gamma))
    newest = (pos + cap - 1) % cap
    idx = np.asarray(idx, np.int64)
    out = dict(k=np.zeros(len(idx), np.int64), last=np.zeros(len(idx), np.int64), rew=np.zeros(len(idx)), done=np.zeros(len(idx)),
               S=np.zeros(len(idx)), rew_norm_bound=np.zeros(len(idx)), kinds=[])
    # every stored reward normalised on its own (rows never stored may hold anything: they are never used below)
    r_hat = np.asarray(ring["rew"], np.float64) if vn is None else normalize_batch64(vn, ring)["rew"]
    for b, i in enumerate(idx):
        t, e = int(i) // N, int(i) % N
        rew = S = nb = 0.0
        kinds = set()
        for j in range(n):
            s = (t + j) % cap
            row = s * N + e
            r = float(r_hat[row])
            rew += g ** j * r
            S += g ** j * abs(r)
            if vn is not None:
                nb += g ** j * float(out_bound(r))
            d = float(ring["done"][row]) != 0.0
            if d or s == newest or j == n - 1:
                break
            if s == cap - 1:
                kinds.add("wraps")                         # the chain goes on from step cap - 1 to step 0
        k = j + 1
        kinds.add("done at newest" if d and s == newest else "cut by done" if d and k < n else "cut at newest" if s == newest and k < n
                  else "full" if not d else "done at n")
        out["k"][b], out["last"][b], out["rew"][b], out["S"][b], out["rew_norm_bound"][b] = k, row, rew, S, nb
        out["done"][b] = 1.0 - g ** (k - 1) * (1.0 - float(ring["done"][row]))
        out["kinds"].append(kinds)
    raw = dict(obs=ring["obs"][idx], act=ring["act"][idx], rew=np.zeros(len(idx)), next_obs=ring["next_obs"][out["last"]], done=out["done"])
    if vn is not None:
        nb64 = normalize_batch64(vn, raw)
        out.update(obs=nb64["obs"], next_obs=nb64["next_obs"])
    else:
        out.update(obs=raw["obs"].astype(np.float64), next_obs=raw["next_obs"].astype(np.float64))
    out["act"] = raw["act"].astype(np.float64)
    return out


def rew_bound(ref):
    """|rew - ref| <= (2k + 1) u S: gamma^j by products is off by up to j u relative, any summation order adds at most (k - 1) u S,
    one final rounding; with a normaliser each term also carries its own rounding to fp32, out_bound(r_j), discounted."""
    return (2 * ref["k"] + 1) * U * ref["S"] + ref["rew_norm_bound"]


def done_bound(ref):
    """|done' - ref| <= (k + 1) u: gamma^(k-1) by products is off by (k - 2) u at most, the product and the difference round once
    each, and every quantity is at most 1."""
    return (ref["k"] + 1) * U


# (N, cap, D, A), the modulus of the done pattern, and the ring states (fill, pos) of the kernel tests
SHAPES = [((3, 7, 5, 2), 4), ((7, 5, 98, 23), 6)]


def states(cap):
    return [(4, 4), (cap, 0), (cap, 3)]


def written_ring(N, cap, D, A, mod, seed=0):
    """A ring written directly: done(s, e) = 1 where (s N + e) mod `mod` = mod - 1, random rewards, observations and actions."""
    rng = np.random.default_rng(seed)
    rows = N * cap
    return dict(obs=rng.standard_normal((rows, D)).astype(np.float32), next_obs=rng.standard_normal((rows, D)).astype(np.float32),
                act=rng.uniform(-1, 1, (rows, A)).astype(np.float32), rew=(2.0 * rng.standard_normal(rows)).astype(np.float32),
                done=(np.arange(rows) % mod == mod - 1).astype(np.float32))
