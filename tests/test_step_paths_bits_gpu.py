"""Everything step_body<TASK> (csrc/dm_kernels.hip) leaves behind, bit for bit against a recording, on every way out of it: the
five launch modes, RSI reset (hash draw, idx_init, mask), RK4 and Euler, the stale-contact-slot bits, every termination with and
without the VecEnv auto-reset, the instability paths, the observation guard, the store-only exit, step_active and the combined
task's motion machine.  The function may be cut into phases or rescheduled; its arithmetic, down to which products the compiler
contracts into FMAs, and its order of effects may not change.

tests/golden/step_paths_bits.npz was recorded on an MI355X by tests/golden/make_step_paths_bits.py from the library as it was
before the first phases were cut out of step_body.  Every case runs sixteen envs on the two-wave kernels and the same envs
tiled to >= 3072 on the three-wave kernels (dm_abi.hip: launch()); tile 0 is kept, after the other tiles were seen to hold the
same bits.  The RSI hash is keyed by the env id, so an env that was reset by a draw differs between the tiles from then on:
those envs are left out of the tile comparison (tile 0 alone has the env ids of the two-wave run).  The two variants need not
equal each other; the file holds the three-wave arrays XORed with the two-wave ones, which is exact and nearly all zeros
(pack / unpack).  The cases are sixteen envs each, not more: the recording has to stay a small file."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_paths_bits.npz")
VARIANTS = ("w2", "w3")                 # two waves per SIMD below 3072 envs, three from there up
TASKS = ("dpenv", "combined")
WALK, RUN, GETUP, TO_GETUP = 0, 1, 2, 3
# include/deepmimic_hip.h
LOW_Z, HIGH_Z, MAX_EP_LEN, ACYCLIC_END, SIM_ERROR, OBS_BOUNDS, FALLEN_NO_AMNESTY = 1, 2, 3, 4, 5, 6, 7
DEBUG_COUNTS = slice(242, 249)          # ncon, nefc, solver_iter, nlimit, overflow, stage ncon bytes, stage nefc bytes
AMNESTY, TO_GETUP_LEN = 150, 180        # dm_default_config
N = 16                                  # envs per case
RESET_MASK = np.tile(np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8), N // 8)


def load_mocaps(model):
    from deepmimic_mujoco_amd.config import MotionConfig
    from deepmimic_mujoco_amd.mocap import MocapDM
    out = {}
    for name in ("walk", "run", "getup_facedown"):
        out[name] = MocapDM(model=model)
        out[name].load_mocap(MotionConfig(name).mocap_path)
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)


class _Run:
    """One engine of n envs (two-wave kernels) or of n envs tiled to >= 3072 (three-wave), and the snapshots taken of it."""

    def __init__(self, model, mocaps, torch, task, variant, sink, n=N, hash_draw=False, **cfg):
        from deepmimic_mujoco_amd import _lib
        self.torch, self.n, self.task, self.sink, self.hash_draw = torch, n, task, sink, hash_draw
        self.same = np.full(n, hash_draw != "reset")    # envs that no hash draw has reset yet, in any tile
        self.tile = 1 if variant == "w2" else -(-3072 // n)
        assert (n * self.tile >= 3072) == (variant == "w3")
        self.eng = eng = _lib.HipEngine(model, n * self.tile, task=TASKS.index(task), **cfg)
        if task == "combined":
            eng.load_clip(0, mocaps["walk"])
            eng.load_clip(1, mocaps["run"])
            eng.load_clip(2, mocaps["getup_facedown"], floor=True, acyclic=True)
        else:                               # one clip under the three flag sets
            eng.load_clip(0, mocaps["walk"])
            eng.load_clip(1, mocaps["walk"], acyclic=True)
            eng.load_clip(2, mocaps["walk"], floor=True)
        self.L = eng.clip_len[0]
        self.out = eng.alloc_outputs()
        self.dbg = eng.enable_debug()

    def dev(self, a, dtype=None):
        a = np.asarray(a)
        t = self.torch.tensor(np.tile(a, (self.tile,) + (1,) * (a.ndim - 1)), device=self.eng.device)
        return (t if dtype is None else t.to(dtype)).contiguous()

    def i32(self, a):
        return self.dev(np.broadcast_to(np.asarray(a, np.int32), (self.n,)), self.torch.int32)

    def ids(self, a):
        """Env ids of tile 0 -> the same envs of every tile; -1 (skipped by the kernel) stays."""
        a = np.asarray(a, np.int32)
        return self.torch.tensor(np.concatenate([np.where(a < 0, a, a + k * self.n) for k in range(self.tile)]),
                                 dtype=self.torch.int32, device=self.eng.device)

    def actions(self, step):
        """fill_random_actions keys on the env id: tile 0's actions for every tile."""
        a = self.torch.zeros(self.n * self.tile, 28, device=self.eng.device)
        self.eng.fill_random_actions(a, step)
        return a[:self.n].repeat(self.tile, 1).contiguous()

    def reset_at(self, frames=None, motions=None):
        if motions is not None:
            self.eng.set_env_clips(self.i32(motions))
        self.eng.reset(self.out["obs"], idx_init=self.i32((np.arange(self.n) * 9 + 2) % self.L if frames is None else frames))

    def state(self):
        """Tile 0's (qpos, qvel, warm, ctrl) as numpy arrays."""
        return [x[:self.n].cpu().numpy() for x in self.eng.get_state()]

    def put(self, q, v, w, c, **kw):
        self.eng.set_state(self.dev(q), self.dev(v), self.dev(w), self.dev(c), **kw)

    def set_root_z(self, z):
        q, v, w, c = self.state()
        q[:, 2] = z
        self.put(q, v, w, c)

    def step(self, k):
        self.eng.step(self.actions(k), self.out)

    def snap(self, label):
        eng = self.eng
        self.torch.cuda.synchronize()
        idx, eplen, eprew = eng.get_counters()
        qpos, qvel, warm, ctrl = eng.get_state()
        fields = dict(self.out, qpos=qpos, qvel=qvel, warm=warm, ctrl=ctrl, idx=idx, eplen=eplen, eprew=eprew,
                      clip=eng.get_env_clips(), work=eng.get_work(), dbg=self.dbg[:, DEBUG_COUNTS])
        if self.hash_draw:      # the auto-reset draws by env id: an env that finished in this launch leaves the comparison
            self.same &= ~(self.out["done"].cpu().numpy().reshape(self.tile, self.n) != 0).any(axis=0)
        for k, x in fields.items():
            a = _bits(x.cpu().numpy()).reshape(self.tile, self.n, -1)
            for t in range(1, self.tile):
                assert np.array_equal(a[0][self.same], a[t][self.same]), "%s %s: tile %d differs from tile 0" % (label, k, t)
            self.sink["%s/%s" % (label, k)] = a[0].copy()

    def close(self):
        self.eng.close()


def _cases(R, task, sink):
    """Runs every case of one task on one kernel variant.  R(**kw) makes a _Run."""
    comb = task == "combined"
    four = [WALK, RUN, GETUP, TO_GETUP] * (N // 4) if comb else None
    tall = np.where(np.arange(N) % 2 == 0, 0.3, 3.0).astype(np.float32)       # root z: below low_z / above high_z

    # ---- reset: hash draw, then a masked second reset (the reset counter moves the draw); idx_init, clamped
    r = R(hash_draw="reset")
    r.eng.reset(r.out["obs"]); r.snap("reset_hash")
    r.eng.reset(r.out["obs"], mask=r.dev(RESET_MASK)); r.snap("reset_masked")
    r.close()
    r = R()
    r.reset_at([-5, -1, 0, 1, r.L - 1, r.L, r.L + 7, 2 * r.L + 3, 2, 17, r.L // 2, r.L - 2, r.L + 1, 3 * r.L, 100000, -2 ** 31], four)
    r.snap("reset_idx")
    r.close()

    # ---- plain steps
    for integ in ("RK4", "Euler"):
        for f8 in (0, 1):
            r = R(integrator=integ, stale_contact_slots=f8, hash_draw=True)
            r.reset_at(motions=four)
            for s in range(3):
                r.step(s); r.snap("plain_%s_f8%d/%d" % (integ, f8, s))
            r.close()

    # ---- terminations, auto-reset on, every env reset twice
    r = R(max_ep_length=2, hash_draw=True)
    r.reset_at(motions=four)
    for s in range(7):
        r.step(s); r.snap("max_ep_len/%d" % s)
    r.close()

    def fall(r, s):     # DPEnv: low / high z.  Combined: walk, fallen, n_steps within the amnesty window
        if comb:
            r.eng.set_env_clips(r.i32(WALK)); r.eng.set_counters(r.i32(np.arange(N) * 9))       # 0 .. 135 <= AMNESTY
        r.set_root_z(tall)
        r.step(s)
    r = R(hash_draw=True)
    r.reset_at()
    for s in range(2):
        fall(r, s); r.snap("z/%d" % s)
    r.close()
    r = R(auto_reset=False)           # a finished env keeps its terminal state
    r.reset_at()
    fall(r, 0); r.snap("z_no_auto_reset/0")
    r.step(1); r.snap("z_no_auto_reset/1")
    r.close()

    if not comb:
        r = R(hash_draw=True)         # clip 1: DM_CLIP_ACYCLIC, the counter two frames before the end
        r.reset_at(motions=[1] * N)
        r.eng.set_counters(r.i32(r.L - 2))
        r.step(0); r.snap("acyclic/0")
        r.step(1); r.snap("acyclic/1")
        r.eng.set_counters(r.i32(r.L - 1))
        r.step(2); r.snap("acyclic/2")
        r.close()
        r = R(hash_draw=True)         # clip 2: DM_CLIP_FLOOR, no z termination
        r.reset_at(motions=[2] * N)
        r.set_root_z(tall)
        for s in range(2):
            r.step(s); r.snap("floor/%d" % s)
        r.close()

    # ---- instability: mj_checkPos / mj_checkVel (non-finite, > 1e10), and a velocity that leaves mj_checkAcc to judge
    def unstable(r):
        r.reset_at(motions=four)
        q, v, w, c = r.state()
        q[1, 10] = np.nan; v[2, 8] = 2e10; v[3, 5] = np.inf; v[4, 7] = 1e7; q[5, 20] = -np.inf
        return q, v, w, c
    r = R(hash_draw=True)
    r.put(*unstable(r)); r.step(0); r.snap("unstable_step")
    r.close()
    r = R()
    q, v, w, c = unstable(r)
    r.eng.step_forced(r.dev(q), r.dev(v), r.out); r.snap("unstable_forced")
    r.close()
    r = R(hash_draw=True)
    r.put(*unstable(r)); r.eng.physics_step(r.actions(0)); r.snap("unstable_physics/0")
    r.step(1); r.snap("unstable_physics/1")
    r.close()

    # ---- observation guard
    r = R(obs_bound=0.5, hash_draw=True)
    r.reset_at(motions=four)
    for s in range(2):
        r.step(s); r.snap("obs_guard/%d" % s)
    r.close()

    # ---- set_state (store only on a permuted subset; with a forward evaluation), forward() alone, step_forced
    r = R()
    r.reset_at(motions=four)
    q, v, w, c = [np.roll(x, 1, axis=0) for x in r.state()]
    w = w + (0.01 * np.arange(34, dtype=np.float32))[None, :]
    c = c + np.float32(0.1)
    sub = [5, 12, 7, 0]
    r.put(q[:4], v[:4], w[:4], c[:4], env_ids=r.ids(sub)); r.snap("set_state_store")
    r.put(q, v, w, c, run_forward=True); r.snap("set_state_forward")
    r.eng.forward(); r.snap("forward")
    r.eng.step_forced(r.dev(np.roll(q, 3, axis=0)), r.dev(np.roll(v, 3, axis=0)), r.out); r.snap("step_forced")
    r.close()

    # ---- step_active on a permuted subset (one entry skipped)
    r = R()
    r.reset_at(motions=four)
    for s, sub in enumerate(([6, 1, -1, 4, 3], [0, 2, 15, 9])):
        ids = r.ids(sub)
        r.eng.step_active(r.actions(s), ids, len(ids), r.out); r.snap("step_active/%d" % s)
    r.close()

    # ---- combined motion machine: four envs just before each transition
    if comb:
        r = R(auto_reset=False)
        Lg = r.eng.clip_len[2]
        walk_frames = [3, 20, 41, 60]
        # states: getup's last frame | walk frames | getup frame 1 (what a to_getup env resets to) | walk frames, then laid low
        r.reset_at([Lg - 1] * 4 + walk_frames + [5, 6, 7, 8] + walk_frames, [GETUP] * 4 + [WALK] * 4 + [TO_GETUP] * 4 + [WALK] * 4)
        q, v, w, c = r.state()
        q[12:, 2] = 0.3
        r.put(q, v, w, c)
        before = np.array([GETUP] * 4 + [TO_GETUP] * 8 + [WALK] * 4, np.int32)
        idx = np.array([Lg - 1] * 4 + [TO_GETUP_LEN - 1] * 4 + [5, 6, 7, 8] + [AMNESTY + 10 + k for k in range(4)], np.int32)
        r.eng.set_env_clips(r.i32(before)); r.eng.set_counters(r.i32(idx))
        sink["machine/motion_before"], sink["machine/idx_before"] = before[:, None], idx[:, None]
        r.eng.step(r.torch.zeros(r.n * r.tile, 28, device=r.eng.device), r.out); r.snap("machine")
        r.close()


def compute(model, mocaps, torch):
    """What the fixture holds, from the library under test: "<variant>/<task>/<case>[/<step>]/<field>" -> int32 [envs, k]
    (fp32 bit patterns, integers as they are)."""
    out = {}
    for variant in VARIANTS:
        for task in TASKS:
            sink = {}
            _cases(lambda **kw: _Run(model, mocaps, torch, task, variant, sink, **kw), task, sink)
            out.update({"%s/%s/%s" % (variant, task, k): a for k, a in sink.items()})
    return out


def pack(arrays):
    """The file's form: the array names without the variant, their shapes, and per variant all arrays end to end, the three-wave
    ones XORed with the two-wave ones."""
    names = sorted(k[3:] for k in arrays if k.startswith("w2/"))
    assert sorted(arrays) == sorted(v + "/" + k for v in VARIANTS for k in names)
    shapes = np.array([arrays["w2/" + k].shape for k in names], np.int32)
    assert all(arrays["w3/" + k].shape == tuple(s) for k, s in zip(names, shapes))
    w2, w3 = (np.concatenate([arrays[v + "/" + k].ravel() for k in names]) for v in VARIANTS)
    return dict(names=np.array(names), shapes=shapes, w2=w2, w3_xor_w2=w3 ^ w2)


def unpack(z):
    flat, out, at = dict(w2=z["w2"], w3=z["w3_xor_w2"] ^ z["w2"]), {}, 0
    for k, (rows, cols) in zip(z["names"], z["shapes"]):
        for v in VARIANTS:
            out["%s/%s" % (v, k)] = flat[v][at:at + rows * cols].reshape(rows, cols)
        at += rows * cols
    return out


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        return unpack({k: z[k] for k in z.files})


@pytest.fixture(scope="module")
def got(model, torch_mod):
    return compute(model, load_mocaps(model), torch_mod)


def _steps(g, prefix, field):
    """[steps, envs] of a one-column field over every snapshot of a case."""
    keys = sorted(k for k in g if k.startswith(prefix) and k.endswith("/" + field))
    assert keys, prefix
    return np.stack([g[k][:, 0] for k in keys])


@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_takes_every_path(golden, variant):
    """The recording holds at least one env on every exit path the cases are there for: each reason code with done set, the
    four motion transitions, a masked-out env on reset and an env that was auto-reset twice."""
    g = golden
    d, c = variant + "/dpenv/", variant + "/combined/"

    def finished(prefix, reason):
        return (_steps(g, prefix, "done") == 1) & (_steps(g, prefix, "reason") == reason)
    high = np.arange(N) % 2 == 1                                                          # the envs lifted above high_z
    for p in (d, c):
        assert (finished(p + "max_ep_len/", MAX_EP_LEN).sum(axis=0) >= 2).any()          # an env auto-reset twice
        assert finished(p + "unstable_step", SIM_ERROR)[0, [1, 2, 3, 5]].all()
        assert finished(p + "unstable_forced", SIM_ERROR)[0, [1, 2, 3, 5]].all()
        assert not finished(p + "unstable_step", SIM_ERROR)[0, [0, 6, 7, 15]].any()
        assert finished(p + "obs_guard/", OBS_BOUNDS).any()
        # a masked-out env is left as it was, the others drew again
        a, b = g[p + "reset_hash/qpos"], g[p + "reset_masked/qpos"]
        keep = RESET_MASK == 0
        assert keep.any() and np.array_equal(a[keep], b[keep]) and (a[~keep] != b[~keep]).any()
        # mj_resetData after an instability in physics mode: qpos0, which no clip frame is
        q = g[p + "unstable_physics/0/qpos"]
        assert np.array_equal(q[1], q[2]) and np.array_equal(q[1], q[3]) and not np.array_equal(q[1], q[0])
        # auto-reset off: done, and the counters run on from the terminal state
        assert (_steps(g, p + "z_no_auto_reset/", "done")[0][high] == 1).all()
        assert (_steps(g, p + "z_no_auto_reset/", "eplen")[1][high] == 2).all()
        # step_active stepped the listed envs and no other
        assert np.array_equal(np.nonzero(g[p + "step_active/0/eplen"][:, 0])[0], [1, 3, 4, 6])
    assert finished(d + "z/", LOW_Z).any() and finished(d + "z/", HIGH_Z)[:, high].all()      # both steps: reset twice
    assert finished(d + "acyclic/", ACYCLIC_END)[1:].all() and not _steps(g, d + "acyclic/", "done")[0].any()
    assert not _steps(g, d + "floor/", "done")[:, high].any() and not _steps(g, d + "floor/", "reason")[:, high].any()
    assert finished(c + "z/", FALLEN_NO_AMNESTY)[:, high].all()
    # the motion machine
    before, idx = g[c + "machine/motion_before"][:, 0], g[c + "machine/idx_before"][:, 0]
    after, done = g[c + "machine/clip"][:, 0], g[c + "machine/done"][:, 0]
    assert ((before == GETUP) & (after == RUN)).any()                                             # getup out of time -> run
    assert ((before == TO_GETUP) & (idx == TO_GETUP_LEN - 1) & (after == GETUP)).any()           # to_getup out of time -> getup
    assert ((before == TO_GETUP) & (idx < TO_GETUP_LEN - 1) & (after == GETUP)).any()            # to_getup -> getup by closeness
    assert ((before == WALK) & (idx > AMNESTY) & (after == TO_GETUP) & (done == 0)).any()        # walk fallen with amnesty -> to_getup


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_paths_bits(got, golden, variant, task):
    """obs, rew, done, terms, reason, terminal_obs, the state (qpos, qvel, warm start, ctrl), the counters, the clip / motion id,
    the work key and debug slots 242..248 after every launch of every case equal the recording bit for bit."""
    prefix = "%s/%s/" % (variant, task)
    keys = sorted(k for k in golden if k.startswith(prefix))
    assert keys and keys == sorted(k for k in got if k.startswith(prefix))
    bad = ["%s (envs %s)" % (k, np.nonzero((got[k] != golden[k]).any(axis=1))[0].tolist()) for k in keys
           if got[k].shape != golden[k].shape or not np.array_equal(got[k], golden[k])]
    assert not bad, "%d of %d arrays differ from the recording: %s" % (len(bad), len(keys), "; ".join(bad[:12]))
