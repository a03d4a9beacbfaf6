"""Batched deterministic evaluation on the device — what `stable_baselines3.common.evaluation.evaluate_policy` [EXT] and the
reference's one-episode-per-point evaluation (src/sb3_ppo.py:25-140; the play scripts' "episode reward > 90" from a chosen start
frame, src/play_g1_run_polar_breeze.py:30-49) do, for N episodes at once.

One evaluation is N episodes, one per env of an ``auto_reset=False`` batch env.  Every episode starts from a chosen reference
frame, acts with the deterministic policy and is stopped at its first ``done`` or at ``max_steps``.  The bookkeeping is one launch
per env step (``dm_eval_advance``, csrc/dm_eval.hip): episode sums in fp64 on the device, finished envs retired, and the ascending
list of the envs still alive rebuilt.  That list is the slot list of ``dm_step_active`` (humanoid3d) and ``dmg1_step_active``
(Unitree G1, both pipelines, both tasks): a finished env — a body lying on the floor, the most expensive kind of env there is
 — is not launched any more, and its state stays what its terminal step left ("frozen").  ``compact`` picks the
engines that take that route (``resolve_compact``): ``True`` the humanoid engines, ``"all"`` every engine that has
``step_active``, the G1 included — what ``evaluation_record`` and with it ``train.py --eval-envs`` and
``EvalDashboardCallback(batch_env=...)`` ask for.  Episode results are bit-identical on either route.  The host reads four bytes
per engine every ``sync_every`` steps and nothing else.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

TRUNCATED = -1      # DM_EVAL_TRUNCATED (include/deepmimic_hip.h): the episode was cut at max_steps, no done flag


@dataclass
class EvalResult:
    """One episode per row.  Tensors (on the env's device when they come from ``BatchEvaluator.run``): ``ep_len`` int32 [n],
    ``ep_ret`` float64 [n] (the fp32 rewards added in step order), ``ep_terms`` float64 [n, terms], ``ep_reason`` int32 [n] (the
    engine's done reason, or ``TRUNCATED``), ``last_obs`` float32 [n, obs] (the observation the terminal step returned),
    ``start_frames`` int32 [n]; ``steps_run`` is the number of env steps the evaluation issued."""
    ep_len: object
    ep_ret: object
    ep_terms: object
    ep_reason: object
    last_obs: object
    start_frames: object
    steps_run: int = 0


# ------------------------------------------------------------------------------------------ host-side arithmetic (no GPU)
def episode_frames(n_episodes, clip_len):
    """``start_frames="all"``: episode e starts at frame e mod L of the clip."""
    return np.arange(int(n_episodes), dtype=np.int64) % int(clip_len)


def plan_rounds(n_episodes, num_envs):
    """[(first episode, episodes)] of the ceil(n_episodes / num_envs) rounds; the last round may leave envs idle."""
    n_episodes, num_envs = int(n_episodes), int(num_envs)
    if n_episodes < 1 or num_envs < 1:
        raise ValueError("n_eval_episodes and num_envs must be >= 1")
    return [(s, min(num_envs, n_episodes - s)) for s in range(0, n_episodes, num_envs)]


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def episode_statistics(results, max_ep_length):
    """The evaluation record over every episode of ``results`` (one ``EvalResult`` or a list, one per round):
    ``episodes``, ``ep_rew_mean``, ``ep_rew_std`` (population, as SB3's ``np.std``), ``ep_len_mean`` and ``frac_reached_cap``,
    the share of episodes that lasted the env's ``MAX_EP_LENGTH`` steps.  An episode cut by a smaller ``max_steps`` did not
    reach the cap: it is the length that counts, not the TRUNCATED reason."""
    if isinstance(results, EvalResult):
        results = [results]
    ret = np.concatenate([_np(r.ep_ret).astype(np.float64).reshape(-1) for r in results])
    ln = np.concatenate([_np(r.ep_len).astype(np.int64).reshape(-1) for r in results])
    return {"episodes": int(ret.size), "ep_rew_mean": float(np.mean(ret)), "ep_rew_std": float(np.std(ret)),
            "ep_len_mean": float(np.mean(ln)), "frac_reached_cap": float(np.mean(ln >= int(max_ep_length)))}


def max_ep_length(env):
    """The env's own episode cap (``ENV_CFG.MAX_EP_LENGTH``: 1000 for DPEnv, 2000 for DPCombinedEnv)."""
    cfg = getattr(env, "ENV_CFG", None)
    if cfg is not None:
        return int(cfg.MAX_EP_LENGTH)
    if is_combined(env):                                               # the G1 batch classes carry no ENV_CFG
        from .combined_env import DPCombinedEnvConfig
        return int(DPCombinedEnvConfig().MAX_EP_LENGTH)
    from .deepmimic_env import DPEnvConfig
    return int(DPEnvConfig().MAX_EP_LENGTH)


def is_combined(env):
    """The env runs the DPCombinedEnv task (either robot)."""
    e = env.engine
    return bool(getattr(e, "task", 0) or getattr(getattr(e, "cfg", None), "task", 0))


def clip_length(env):
    """Frames of the env's clip 0 (what ``start_frames="all"`` walks through)."""
    L = env.engine.clip_len
    return int(L[0] if isinstance(L, dict) else L)


def resolve_compact(compact, humanoid):
    """Whether ``BatchEvaluator(compact=...)`` launches only the live envs, on an env whose engines are all humanoid3d
    (``humanoid`` true) or not (Unitree G1): ``True`` compacts the humanoid engines alone, ``"all"`` every engine that has
    ``step_active``, ``False`` none.  Anything else is a ``ValueError``."""
    if isinstance(compact, str) and compact == "all":
        return True
    if isinstance(compact, (bool, np.bool_)):
        return bool(compact) and bool(humanoid)
    raise ValueError("compact is True (humanoid3d engines only), \"all\" (every engine) or False, not %r" % (compact,))


# ------------------------------------------------------------------------------------------ the evaluator
class BatchEvaluator:
    """``run`` = one episode per env of ``env`` (any ``HipBatchEnv`` built with ``auto_reset=False``, any ``sub_batches``).

    ``compact`` (``resolve_compact``): ``True`` launches only the envs still alive on the humanoid3d engines
    (``dm_step_active``), ``"all"`` on the Unitree G1 engines too (``dmg1_step_active``; with ``sub_batches > 1`` each engine on
    its own stream, as the env's own step).  A finished env's engine state then stays what its terminal step left.  Everything
    else — ``compact=False``, a G1 env under ``True`` — steps all envs with the plain ``step_tensor`` and only the bookkeeping
    ignores the finished ones (their engine state moves on; nothing reads it).  The episodes are the same bit for bit.
    ``sync_every``: env steps between two reads of the live count; the results do not depend on it."""

    def __init__(self, env, compact=True, sync_every=16):
        if getattr(env, "auto_reset", True):
            raise ValueError("BatchEvaluator needs an env built with auto_reset=False: an auto-resetting env starts a new episode "
                             "inside the step that ends one, so there is no terminal state to stop at")
        if int(sync_every) < 1:
            raise ValueError("sync_every must be >= 1")
        import torch
        self.torch, self.env = torch, env
        self.sync_every = int(sync_every)
        from ._lib import HipEngine
        self.humanoid = all(isinstance(e, HipEngine) for e in env.engines)
        self.compact = resolve_compact(compact, self.humanoid)
        if self.compact and not all(hasattr(e, "step_active") for e in env.engines):
            raise ValueError("compact=%r: an engine of this env has no step_active" % (compact,))
        self.N, self.device = int(env.num_envs), env.device
        self.obs_dim, self.terms_dim = int(env.out["obs"].shape[1]), int(env.out["terms"].shape[1])
        self.launched_env_steps = 0        # env steps handed to the step kernels by the last run (an upper bound under compaction)
        N, dev = self.N, self.device
        z = lambda *shape, dt: torch.zeros(*shape, dtype=dt, device=dev)
        self.alive, self.ep_len, self.ep_reason = z(N, dt=torch.uint8), z(N, dt=torch.int32), z(N, dt=torch.int32)
        self.ep_ret, self.ep_terms = z(N, dt=torch.float64), z(N, self.terms_dim, dt=torch.float64)
        self.last_obs = z(N, self.obs_dim, dt=torch.float32)
        self.env_ids = z(N, dt=torch.int32)                    # per engine slice: LOCAL env indices, ascending, -1 tail
        self.counts = z(len(env.engines), dt=torch.int32)

    def _clear_carry_over(self):
        """A reset keeps the warm start and the controls of whatever the env ran before, as ``MjSim.set_state`` does in the reference,
        and its forward evaluation starts from them: the first steps of an episode would differ in the last bits from one evaluation
        to the next.  Both are cleared first, so an evaluation is a function of the policy and the start frames alone and equals a
        run on a freshly built env.  The humanoid engine takes both through ``set_state``; the G1 engine's ``set_state`` has no
        controls, there one step with zero actions (from a reset state) puts them to zero."""
        t = self.torch
        for e, o, sl in zip(self.env.engines, self.env.sub_out, self.env.sub_slices):
            if self.humanoid:
                q, v, w, c = e.get_state()
                e.set_state(q, v, warm=t.zeros_like(w), ctrl=t.zeros_like(c), run_forward=False)
            else:
                e.reset(o["obs"])        # a defined state to step from: a freshly built engine has never been reset
                e.step(t.zeros(sl.stop - sl.start, self.env.action_space.shape[0], device=self.device), o)
                q, v, w = e.get_state()
                e.set_state(q, v, warm=t.zeros_like(w), run_forward=False)

    def _advance(self, max_steps):
        from . import _lib
        out, dev_index = self.env.out, self.device.index or 0
        for k, sl in enumerate(self.env.sub_slices):
            _lib.call("dm_eval_advance", sl.stop - sl.start, self.terms_dim, int(max_steps), out["rew"][sl], out["done"][sl],
                      out["reason"][sl], out["terms"][sl], out["obs"][sl], self.obs_dim, self.alive[sl], self.ep_len[sl],
                      self.ep_ret[sl], self.ep_terms[sl], self.ep_reason[sl], self.last_obs[sl], self.env_ids[sl],
                      self.counts[k:k + 1], dev_index, device=self.device)

    def _step_active(self, actions, nslots):
        """One step of the live envs of every engine.  A G1 env of several engines forks each engine's launches onto that
        engine's stream and joins them back, as ``HipG1VecEnv._step_engines`` does for the plain step."""
        t, env = self.torch, self.env
        work = [x for x in zip(env.engines, env.sub_out, env.sub_slices, nslots) if x[3] > 0]
        if self.humanoid or len(env.engines) == 1:
            for e, o, sl, ns in work:
                e.step_active(actions[sl], self.env_ids[sl], ns, o)
            return
        cur = t.cuda.current_stream(self.device)
        if getattr(env, "_streams", None) is None:
            from .streams import concurrent_streams
            env._streams = concurrent_streams(self.device, len(env.engines))
        fork = cur.record_event()
        for (e, o, sl, ns), s in zip(work, [env._streams[k] for k, ns in enumerate(nslots) if ns > 0]):
            s.wait_event(fork)
            with t.cuda.stream(s):
                e.step_active(actions[sl], self.env_ids[sl], ns, o)
            cur.wait_event(s.record_event())

    def run(self, act_fn, start_frames=None, max_steps=None):
        """``act_fn(obs [N, D]) -> actions [N, A]`` on device tensors (all N rows, every step; rows of finished envs are ignored).
        ``start_frames``: int array of n <= N frames, episode i on env i (envs from n on stay idle); ``None`` = the engine's own
        seeded reference-state initialisation on all N envs, the only mode of the combined task (whose ``idx_init`` is
        ``n_steps``).  ``max_steps=None``: the env's ``MAX_EP_LENGTH``."""
        with self.torch.no_grad():
            return self._run(act_fn, start_frames, max_steps)

    def _run(self, act_fn, start_frames, max_steps):
        t, env, N = self.torch, self.env, self.N
        max_steps = max_ep_length(env) if max_steps is None else int(max_steps)
        if max_steps < 1:
            raise ValueError("max_steps must be >= 1")
        if start_frames is None:
            n, idx_init = N, None
        else:
            if is_combined(env):
                raise ValueError("the combined task has no start frames (its idx_init is n_steps): pass start_frames=None")
            sf = t.as_tensor(np.asarray(_np(start_frames)).astype(np.int32).reshape(-1), device=self.device)
            n = int(sf.numel())
            if not 1 <= n <= N:
                raise ValueError("start_frames holds %d frames for %d envs" % (n, N))
            idx_init = t.zeros(N, dtype=t.int32, device=self.device)
            idx_init[:n] = sf
        self._clear_carry_over()
        obs = env.reset_tensor(idx_init)
        if idx_init is None:
            idx_init = t.cat([e.get_counters()[0] for e in env.engines])
        for buf in (self.ep_len, self.ep_reason, self.ep_ret, self.ep_terms, self.last_obs):
            buf.zero_()
        self.alive.copy_((t.arange(N, device=self.device) < n).to(t.uint8))
        nslots = []
        for k, sl in enumerate(env.sub_slices):
            nk = sl.stop - sl.start
            live = max(0, min(nk, n - sl.start))
            local = t.arange(nk, dtype=t.int32, device=self.device)
            self.env_ids[sl] = t.where(local < live, local, t.full_like(local, -1))
            nslots.append(live)
        steps = launched = 0
        while steps < max_steps:
            actions = act_fn(obs)
            if self.compact:
                self._step_active(actions.contiguous(), nslots)
                launched += sum(nslots)
            else:
                env.step_tensor(actions)
                launched += N
            self._advance(max_steps)
            steps += 1
            if steps % self.sync_every == 0 and steps < max_steps:
                nslots = [int(c) for c in self.counts.tolist()]        # the one host read: 4 bytes per engine
                if sum(nslots) == 0:
                    break
        self.launched_env_steps = launched
        c = lambda x: x[:n].clone()
        return EvalResult(ep_len=c(self.ep_len), ep_ret=c(self.ep_ret), ep_terms=c(self.ep_terms), ep_reason=c(self.ep_reason),
                          last_obs=c(self.last_obs), start_frames=c(idx_init), steps_run=steps)


# ------------------------------------------------------------------------------------------ the action route of a model
def policy_act_fn(model, env, deterministic=True):
    """``act_fn`` of ``BatchEvaluator.run`` for the supported policy types.

    ``ppo.PPO``: ``dm_policy_forward`` with ``deterministic=1`` where ``FusedPolicyForward.supported`` — its ``act_env`` output is
    the clamped action ``collect_rollouts`` hands to the env — with the weights packed now (call again after training went on);
    ``model.predict`` otherwise.  ``sac.SAC``: ``model.predict(deterministic=True)``.  ``ppo.ExtractedPolicy``: the reference's
    protocol, ``clip(act(obs[:, :66]), -0.5, 0.5)`` (src/play_extracted.py:36-38).  Any other callable is passed through.
    ``deterministic=False`` is refused on the fused PPO route (a stochastic evaluation would have to share the rollout's draw
    counter; nothing needs it yet); ``predict`` takes the flag as it is."""
    import torch
    from .ppo import PPO, ExtractedPolicy, FusedPolicyForward
    from .sac import SAC
    dev = env.device
    if isinstance(model, PPO):
        if model.device.type == "cuda" and model.fused_policy and FusedPolicyForward.supported(model.policy, model.device):
            if not deterministic:
                raise ValueError("the fused PPO route evaluates the deterministic policy only (deterministic=False is not implemented)")
            fwd = FusedPolicyForward(model.policy, model.device)
            fwd.pack()
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            bufs = {}

            def act(obs):
                n = obs.shape[0]
                if n not in bufs:
                    z = lambda *s: torch.zeros(*s, device=dev)
                    bufs[n] = (z(n, fwd.A), z(n, fwd.A), z(n), z(n))
                a, a_env, logp, val = bufs[n]
                fwd(obs.contiguous(), 0, counter, 0, model.act_lo, model.act_hi, a, a_env, logp, val, deterministic=True)
                return a_env
            return act
        return lambda obs: model.predict(obs, deterministic=deterministic)
    if isinstance(model, SAC):
        return lambda obs: model.predict(obs, deterministic=deterministic)
    if isinstance(model, ExtractedPolicy):
        import copy
        pol = copy.copy(model)
        pol.p = {k: v.to(dev) for k, v in model.p.items()}
        return lambda obs: torch.clamp(pol.act(obs[:, :pol.obs_shape]), -0.5, 0.5)
    if callable(model):
        return model
    raise TypeError("policy_act_fn: a PPO, SAC, ExtractedPolicy or a callable obs -> actions, not %r" % type(model).__name__)


# ------------------------------------------------------------------------------------------ SB3's contract
def is_multi_clip(env):
    """The envs of the batch follow different clips (``motion`` was a list): there is no one set of "all" start frames."""
    return len(getattr(env, "motions", None) or ()) > 1


def resolve_frames(env, n_eval_episodes, start_frames):
    """``(episodes, frames)`` of ``run_episodes``: ``frames[e]`` is episode e's start frame, or ``frames`` is None for the engine's
    seeded random frames.  ``"all"`` walks through clip 0 and is refused on a multi-clip env, whose envs follow clips of different
    lengths: pass an explicit array or None there."""
    if isinstance(start_frames, str):
        if start_frames != "all":
            raise ValueError("start_frames is \"all\", an int array or None")
        if is_multi_clip(env):
            raise ValueError("start_frames=\"all\" needs a single-clip env (this one mixes %d clips): pass an int array or None" % len(env.motions))
        L = clip_length(env)
        n_eval_episodes = L if n_eval_episodes is None else int(n_eval_episodes)
        return n_eval_episodes, episode_frames(n_eval_episodes, L)
    if start_frames is None:
        return (env.num_envs if n_eval_episodes is None else int(n_eval_episodes)), None
    given = np.asarray(_np(start_frames)).astype(np.int64).reshape(-1)
    n_eval_episodes = given.size if n_eval_episodes is None else int(n_eval_episodes)
    return n_eval_episodes, given[np.arange(n_eval_episodes) % given.size]


def normalized_act_fn(act_fn, normalizer):
    """``act_fn`` behind a ``vec_normalize.HipVecNormalize``'s frozen transform: the policy sees ``normalizer.normalize_obs(obs)``
    (``dm_vecnorm_apply``, one launch for however many rows); the statistics are only read."""
    if normalizer is None:
        return act_fn
    return lambda obs: act_fn(normalizer.normalize_obs(obs))


def run_episodes(model, env, n_eval_episodes=None, start_frames="all", deterministic=True, max_steps=None, compact=True,
                 sync_every=16, normalizer=None):
    """The rounds behind ``evaluate_policy``: a list of ``EvalResult``, one per round of at most ``env.num_envs`` episodes.
    ``start_frames``: ``"all"`` (episode e from frame e mod L of a single-clip env's clip; ``n_eval_episodes`` defaults to L), an int array
    (episode e from ``start_frames[e mod len]``; defaults to its length) or ``None`` (the engine's seeded random frames;
    defaults to ``env.num_envs``).  ``normalizer``: a ``HipVecNormalize`` whose frozen statistics transform the observations the
    policy sees (``env`` itself stays unwrapped, so the episode returns are raw).  The episodes of several rounds equal those of one large batch bit for bit only if ``act_fn``
    computes a row's action independently of the number of rows; a library GEMM does not promise that."""
    n_eval_episodes, frames = resolve_frames(env, n_eval_episodes, start_frames)
    ev = BatchEvaluator(env, compact=compact, sync_every=sync_every)
    act_fn = normalized_act_fn(policy_act_fn(model, env, deterministic=deterministic), normalizer)
    results = []
    for first, cnt in plan_rounds(n_eval_episodes, env.num_envs):
        if frames is None:
            r = ev.run(act_fn, None, max_steps)
            if cnt < env.num_envs:
                r = EvalResult(*[getattr(r, f)[:cnt] for f in ("ep_len", "ep_ret", "ep_terms", "ep_reason", "last_obs", "start_frames")],
                               steps_run=r.steps_run)
        else:
            r = ev.run(act_fn, frames[first:first + cnt], max_steps)
        results.append(r)
    return results


def evaluate_policy(model, env, n_eval_episodes=None, start_frames="all", deterministic=True, max_steps=None,
                    return_episode_rewards=False, compact=True, normalizer=None):
    """``stable_baselines3.common.evaluation.evaluate_policy`` [EXT] on a batch env: ``(mean_reward, std_reward)``, or with
    ``return_episode_rewards`` the lists ``(episode_rewards, episode_lengths)`` in episode order.  When there are more episodes than
    envs the evaluator runs ceil(episodes / num_envs) rounds.  See ``run_episodes`` for ``start_frames``, ``BatchEvaluator``
    for ``compact`` (``"all"`` also leaves finished Unitree G1 envs out of the launches; same numbers) and for ``normalizer``."""
    results = run_episodes(model, env, n_eval_episodes, start_frames, deterministic, max_steps, compact, normalizer=normalizer)
    if return_episode_rewards:
        return ([float(x) for r in results for x in _np(r.ep_ret)], [int(x) for r in results for x in _np(r.ep_len)])
    s = episode_statistics(results, max_ep_length(env))
    return s["ep_rew_mean"], s["ep_rew_std"]


def evaluation_record(model, env, global_step, start_frames="all", n_eval_episodes=None, max_steps=None, compact="all", normalizer=None):
    """The six fields of one evaluation point (``eval_batch.csv`` of ``EvalDashboardCallback``, ``"eval"`` of ``train.py --json``).
    ``compact="all"``: finished envs leave the launches on either robot (DESIGN §16 has the measurement behind the default)."""
    if is_combined(env) or (isinstance(start_frames, str) and is_multi_clip(env)):
        start_frames = None                                    # the combined task and a multi-clip env start from seeded random states
    results = run_episodes(model, env, n_eval_episodes, start_frames, True, max_steps, compact, normalizer=normalizer)
    return dict({"global_step": int(global_step)}, **episode_statistics(results, max_ep_length(env)))


RECORD_FIELDS = ("global_step", "episodes", "ep_rew_mean", "ep_rew_std", "ep_len_mean", "frac_reached_cap")
