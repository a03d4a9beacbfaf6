"""The constraint stage of dm_step_kernel (fwd_collide, fwd_constraint: csrc/dm_kernels.hip) and of the G1 engine, pinned path by
path against the fp64 oracle on the states of tests/constraint_path_states.py: every row-count path and the boundaries between
them (nefc 0 | 1..7 | 8..32 | 33..64 | 65..128), the 32-contact and the 128-row cap (G1: 48 / 256) with the overflow flag, limit
rows on either side of every joint, both transposes of the force tail, warm start kept / discarded, PGS leaving early / late.
tests/test_constraint_paths_cpu.py shows, without a GPU, that the states really are all that."""
import numpy as np
import pytest

import constraint_path_states as cps

pytestmark = pytest.mark.gpu

TOL_QPOS = 1e-4          # per-step qpos L-inf, as tests/test_gpu_parity.py
TOL_DIST = 2e-6          # contact distance, as test_narrowphase_coverage_all_pair_types
TOL_QACC = {False: 2e-3, True: 5e-3}      # relative to max(1, |qacc|inf): <= 64 rows / the wide path (test_gpu_parity.py)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def states(model):
    return cps.humanoid_states(model)


def _engine(model, clips, n):
    from deepmimic_mujoco_amd._lib import HipEngine
    eng = HipEngine(model, n, auto_reset=False)
    eng.load_clip(0, clips["walk"])
    return eng


def _put(eng, torch, H, tile):
    t = lambda a: torch.tensor(np.tile(a, (tile, 1)), dtype=torch.float32, device=eng.device).contiguous()
    eng.set_state(t(H["qpos"]), t(H["qvel"]), t(H["warm"]), torch.zeros(len(H["qpos"]) * tile, 28, device=eng.device))


def _forward(model, clips, torch, H, tile=1):
    """set_state(q, v, warm, ctrl = 0), forward(): the debug rows [tile, states, DM_DEBUG_STRIDE]."""
    n = len(H["qpos"])
    eng = _engine(model, clips, n * tile)
    _put(eng, torch, H, tile)
    dbg = eng.enable_debug()
    eng.forward()
    torch.cuda.synchronize()
    d = dbg.cpu().numpy().reshape(tile, n, -1).copy()
    eng.close()
    return d


PATHS = ("0", "1..7", "8..32", "33..64", "65..128", "cut")


def _path(lab):
    if lab["cut_con"] or lab["cut_row"]:
        return "cut"
    n = lab["nefc"]
    return "0" if n == 0 else "1..7" if n < 8 else "8..32" if n <= 32 else "33..64" if n <= 64 else "65..128"


def _check_forward(d, H):
    """One debug row per state against the oracle; every failure names the state."""
    worst = {p: dict(n=0, qacc=0.0, cons=0.0, force=0.0, dist=0.0) for p in PATHS}
    skipped = compared = 0
    for i, lab in enumerate(H["labels"]):
        ref, name, row = lab["ref"], "state %d, %s" % (i, cps.describe(lab)), d[i]
        w = worst[_path(lab)]
        w["n"] += 1
        # ---- exact: contact list in order, row counts, limit rows, the overflow flag bit by bit
        ncon = int(row[242])
        assert ncon == lab["ncon"], name
        gpu = [(int(row[256 + 3 * c]), int(row[257 + 3 * c])) for c in range(ncon)]
        assert gpu == [(int(c[13]), int(c[14])) for c in ref["contact"]], name
        assert int(row[243]) == lab["nefc"], (name, row[243])
        assert int(row[245]) == lab["nlimit"], (name, row[245])
        flag = int(row[246])
        assert row[246] == flag and (flag & 1, (flag >> 1) & 1, flag >> 2) == (int(lab["cut_con"]), int(lab["cut_row"]), 0), (name, flag)
        # ---- contact distance
        if ncon:
            w["dist"] = max(w["dist"], np.abs(row[258:258 + 3 * ncon:3] - ref["contact"][:, 0]).max())
            assert w["dist"] < TOL_DIST, name
        # ---- qacc, and its constraint part alone (a large qacc_smooth must not hide a solver error)
        tol = TOL_QACC[lab["nefc"] > 64]
        scale = max(1.0, np.abs(ref["qacc"]).max())
        e_qacc = np.abs(row[174:208] - ref["qacc"]).max() / scale
        e_cons = np.abs((row[174:208].astype(np.float64) - row[208:242]) - (ref["qacc"] - ref["qacc_smooth"])).max() / scale
        w["qacc"], w["cons"] = max(w["qacc"], e_qacc), max(w["cons"], e_cons)
        assert e_qacc < tol, (name, e_qacc)
        assert e_cons < tol, (name, e_cons)
        if lab["nefc"] == 0:
            assert np.array_equal(row[174:208], row[208:242]), name
        # ---- row forces (exported up to 64 rows): none beyond nefc, none negative, and M^-1 J^T (f_gpu - f_oracle) in fp64
        if 0 < lab["nefc"] <= 64:
            f = row[352:416].astype(np.float64)
            assert np.all(f[lab["nefc"]:] == 0), name
            assert np.all(f >= 0), name
            e_f = np.abs(np.linalg.solve(ref["M"], ref["J"].T @ (f[:lab["nefc"]] - ref["force"]))).max() / scale
            w["force"] = max(w["force"], e_f)
            assert e_f < tol, (name, e_f)
        # ---- sweeps, where the oracle's own count does not hang on the last digit of the tolerance
        if lab["nefc"] == 0:
            assert int(row[244]) == 0, name
        elif lab["stable"]:
            compared += 1
            assert int(row[244]) == lab["sweeps"], (name, row[244])
        else:
            skipped += 1
    print("   path      states  qacc      constraint part  M^-1 J^T df  contact dist")
    for p in PATHS:
        w = worst[p]
        print("   %-9s %5d   %.2e  %.2e         %.2e     %.2e" % (p, w["n"], w["qacc"], w["cons"], w["force"], w["dist"]))
    print("   sweep counts compared on %d states, skipped on %d (oracle count moves with its tolerance x 0.9 / x 1.1)" % (compared, skipped))
    return worst


def test_forward_evaluation_on_every_constraint_path(model, clips, torch_mod, states):
    """dm_step_kernel (two waves per SIMD) on the generator's states: contact list, nefc, nlimit and the overflow bits exactly;
    contact distance 2e-6; qacc and qacc - qacc_smooth to 2e-3 (<= 64 rows) / 5e-3 (wide path) of max(1, |qacc|inf), cut states
    included; exported row forces zero past nefc, non-negative, and M^-1 J^T (f - f_oracle) inside the same gate; sweep counts
    equal wherever the oracle's count is stable."""
    d = _forward(model, clips, torch_mod, states)
    assert len(states["labels"]) < 3072
    _check_forward(d[0], states)


def test_forward_evaluation_on_every_path_three_wave_kernel(model, clips, torch_mod, states):
    """The same states tiled to >= 3072 envs, where dm_step_kernel_w3 runs: the same gates, and every tile bit-identical."""
    n = len(states["labels"])
    tile = -(-3072 // n)
    d = _forward(model, clips, torch_mod, states, tile=tile)
    assert d.shape[0] * d.shape[1] >= 3072
    for k in range(1, tile):
        assert np.array_equal(d[0].view(np.int32), d[k].view(np.int32)), "tile %d differs from tile 0" % k
    _check_forward(d[0], states)


def test_dynamic_step_from_cut_and_boundary_states(model, clips, torch_mod, states):
    """One RK4 step (zero action) from every cut state and every state on a path boundary, against OracleSim.step(): contact and
    row counts of all four stages identical, qpos L-inf < 1e-4.  No exclusion set."""
    from oracle.oracle import OracleSim
    torch = torch_mod
    pick = [i for i, lab in enumerate(states["labels"])
            if lab["cut_con"] or lab["cut_row"] or lab["nefc"] in cps.BOUNDARY_NEFC + cps.TOP_NEFC]
    H = dict(qpos=states["qpos"][pick], qvel=states["qvel"][pick], warm=states["warm"][pick])
    labels = [states["labels"][i] for i in pick]
    assert sum(1 for x in labels if x["cut_con"] or x["cut_row"]) >= 12 and len(labels) >= 60
    eng = _engine(model, clips, len(pick))
    _put(eng, torch, H, 1)
    dbg = eng.enable_debug()
    out = eng.alloc_outputs()
    eng.step(torch.zeros(len(pick), 28, device=eng.device), out)
    torch.cuda.synchronize()
    qg = eng.get_state()[0].double().cpu().numpy()
    packs = dbg.cpu().numpy()[:, 247:249].copy().view(np.int32)
    eng.close()
    s = OracleSim(model)
    s.set_caps(cps.MAXCON, cps.MAXROW)
    worst, flips = 0.0, []
    for i, lab in enumerate(labels):
        s.set("qpos", H["qpos"][i]); s.set("qvel", H["qvel"][i]); s.set("qacc_warmstart", H["warm"][i]); s.set("ctrl", np.zeros(28))
        assert s.step() == 0
        ora = ([s.geti("stage_ncon%d" % k) for k in range(4)], [s.geti("stage_nefc%d" % k) for k in range(4)])
        gpu = ([(int(packs[i, 0]) >> (8 * k)) & 0xFF for k in range(4)], [(int(packs[i, 1]) >> (8 * k)) & 0xFF for k in range(4)])
        err = np.abs(qg[i] - s.get("qpos")).max()
        if gpu != ora:
            flips.append((pick[i], cps.describe(lab), gpu, ora))
            print("   stage counts differ:", flips[-1])
        worst = max(worst, err)
        assert err < TOL_QPOS or gpu != ora, (cps.describe(lab), err)
    print("   one step from %d cut / boundary states: qpos max err %.3g, stage-count differences %d" % (len(pick), worst, len(flips)))
    assert not flips, flips
    assert worst < TOL_QPOS


# ---------------------------------------------------------------------------------------------------------------- Unitree G1
@pytest.fixture(scope="module")
def g1(torch_mod):
    """The G1 states (contact-cut, controls, row-cut), the oracle's answers, and the debug rows of both pipelines."""
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    from oracle import oracle_g1 as og
    torch = torch_mod
    G = cps.g1_states(row_cut_draws=200)
    n = len(G["labels"])
    ora = []
    for q, v in zip(G["qpos"], G["qvel"]):
        s = og.G1Sim()
        s.set_caps(cps.G1_MAXCON, cps.G1_MAXROW)
        assert s.set_state(q, v) == 0
        ora.append(dict(contacts=s.contacts(), nefc=s.geti("nefc"), nlimit=s.geti("nlimit"), qacc=s.get("qacc"),
                        cut=s.geti("overflow_con") > 0 or s.geti("overflow_row") > 0))
    dbg = {}
    for pl in (1, 2):
        eng = G1HipEngine(n, auto_reset=False, pipeline=pl)
        eng.load_clip(cps.g1_mocap("walk"))
        buf = eng.enable_debug()
        dev = eng.device
        eng.set_state(torch.tensor(G["qpos"], dtype=torch.float32, device=dev).contiguous(),
                      torch.tensor(G["qvel"], dtype=torch.float32, device=dev).contiguous(), torch.zeros(n, 43, device=dev))
        torch.cuda.synchronize()
        dbg[pl] = buf.cpu().numpy().copy()
        eng.close()
    return G, ora, dbg


@pytest.mark.parametrize("pipeline", [1, 2])
def test_g1_forward_evaluation_at_the_caps(g1, pipeline):
    """G1HipEngine, monolithic and split pipeline, on states cut by the 48-contact cap, on uncut controls of 40..48 contacts and
    on states cut by the 256-row cap: the contact list is the oracle's (geoms in order, dist 1e-6, pos 1e-5, normal 1e-5), the
    overflow flag is set exactly on the cut states, row counts equal, qacc within 5e-3."""
    G, ora, dbg = g1
    worst = dict(cdist=0.0, cpos=0.0, cnrm=0.0, qacc=0.0)
    for i, (lab, o) in enumerate(zip(G["labels"], ora)):
        d, name = dbg[pipeline][i], "G1 state %d (%s, %d contacts, %d rows)" % (i, lab["kind"], lab["ncon"], lab["nefc"])
        ncon = int(d[203])
        c = d[208:208 + 9 * ncon].reshape(-1, 9)
        assert ncon == len(o["contacts"]) == lab["ncon"], (name, ncon)
        assert [(int(r[1]), int(r[2])) for r in c] == [(k["geom1"], k["geom2"]) for k in o["contacts"]], name
        for r, k in zip(c, o["contacts"]):
            worst["cdist"] = max(worst["cdist"], abs(r[0] - k["dist"]))
            worst["cpos"] = max(worst["cpos"], np.abs(r[3:6] - k["pos"]).max())
            worst["cnrm"] = max(worst["cnrm"], np.abs(r[6:9] - k["frame"][0]).max())
        assert worst["cdist"] < 1e-6 and worst["cpos"] < 1e-5 and worst["cnrm"] < 1e-5, (name, worst)
        assert int(d[207]) == int(lab["kind"] != "control") == int(o["cut"]), (name, d[207])
        assert (int(d[204]), int(d[206])) == (o["nefc"], o["nlimit"]), (name, d[204], d[206], o["nefc"], o["nlimit"])
        e = np.abs(d[160:203] - o["qacc"]).max() / max(1.0, np.abs(o["qacc"]).max())
        worst["qacc"] = max(worst["qacc"], e)
        assert e < 5e-3, (name, e)
    print("   G1 pipeline %d at the caps:" % pipeline, {k: float(v) for k, v in worst.items()})


def test_g1_pipelines_bit_identical_at_the_caps(g1):
    """Monolithic kernel and split pipeline leave the same bits on every one of these states: body poses, both accelerations,
    counts, flag, the contact list and the row forces (slots 900..915 hold per-kernel timing marks and are left out)."""
    G, ora, dbg = g1
    a, b = dbg[1].view(np.int32), dbg[2].view(np.int32)
    for i, lab in enumerate(G["labels"]):
        assert np.array_equal(a[i, :900], b[i, :900]), ("G1 state %d (%s)" % (i, lab["kind"]), np.nonzero(a[i, :900] != b[i, :900])[0][:8])


@pytest.mark.parametrize("pipeline", [1, 2])
def test_g1_teacher_forced_step_from_the_cut_states(g1, torch_mod, pipeline):
    """One step of small random torques from the contact-cut and row-cut states against the oracle's step of the same state: the
    contact list of every RK stage by count and by hash, every stage's row count, and qpos L-inf < 1e-4."""
    from deepmimic_mujoco_amd.g1 import G1HipEngine
    from oracle import oracle_g1 as og
    torch = torch_mod
    G = g1[0]
    pick = [i for i, lab in enumerate(G["labels"]) if lab["kind"] != "control"]
    n = len(pick)
    mc = cps.g1_mocap("walk")
    clip = og.G1Clip(*mc.tables())
    eng = G1HipEngine(n, auto_reset=False, pipeline=pipeline)
    eng.load_clip(mc)
    out = eng.alloc_outputs()
    eng.reset(out["obs"], idx_init=torch.zeros(n, dtype=torch.int32, device=eng.device))
    dbg = eng.enable_debug()
    dev = eng.device
    eng.set_state(torch.tensor(G["qpos"][pick], dtype=torch.float32, device=dev).contiguous(),
                  torch.tensor(G["qvel"][pick], dtype=torch.float32, device=dev).contiguous(), torch.zeros(n, 43, device=dev),
                  run_forward=False)
    act = (np.random.default_rng(3).uniform(-1, 1, (n, 23)) * 0.05).astype(np.float32)
    eng.step(torch.tensor(act, device=dev), out)
    torch.cuda.synchronize()
    q2 = eng.get_state()[0].cpu().numpy()
    d = dbg.cpu().numpy()
    eng.close()
    worst = 0.0
    for j, i in enumerate(pick):
        name = "G1 state %d (%s)" % (i, G["labels"][i]["kind"])
        s = og.G1Sim()
        s.set_caps(cps.G1_MAXCON, cps.G1_MAXROW)
        s.env_reset(clip, 0)
        s.set("qpos", G["qpos"][i]); s.set("qvel", G["qvel"][i]); s.set("qacc_warmstart", np.zeros(43))
        s.env_step(clip, act[j].astype(np.float64))
        for k in range(4):
            assert (int(d[j][1000 + k]), int(d[j][1012 + k])) == (s.geti("stage_ncon%d" % k), s.geti("stage_chash%d" % k)), \
                ("contact list of RK stage %d differs" % k, name)
            assert int(d[j][1004 + k]) == (s.geti("stage_nefc%d" % k) & 0xFF), ("row count of RK stage %d differs" % k, name)
        worst = max(worst, np.abs(q2[j] - s.get("qpos")).max())
    print("   G1 pipeline %d, one step from %d cut states: qpos max err %.3g" % (pipeline, n, worst))
    assert worst < 1e-4
