"""SHA-256 digests of what one call of each wide learner (dm_ppo_wide_grad: one bf16 plane per array; dm_ppo_wide3_grad: two) leaves
behind, for comparing two builds of the library bit for bit.

Public C ABI through ``_lib`` only, so the same file runs against any build that has the two entry points (``DM_LIB_VARIANT=x``
loads ``libdeepmimic_hip_x.so`` next to the shipped library, as bench_learner.py does).  Per entry point and shape (the six of
tests/ppo_wide_ref64.SHAPES): seeded inputs, zero-filled scratch, one call with the folds on, then a digest of each of: both trunks'
packed weights, xbT, h1T, h2T, dz3T, dz2T, dz1T, part, stats8, out8, g_log_std, and at 1024x512-d67-a28-b256 (split-K 1 in every
job: fixed summation order) the six weight gradients.  Bias gradients and weight gradients with split-K > 1 go through fp32 atomics
and are left out.

    python scripts/wide_digest.py --out digest.json
    python scripts/wide_digest.py --compare a.json b.json        # lists the differing entries; exit status 1 if there are any
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {   # name: (H1, H2, D, A, B, normalize, ent_coef)
    "256x128-d1-a1-b64": (256, 128, 1, 1, 64, False, 0.0),
    "256x128-d85-a23-b1024": (256, 128, 85, 23, 1024, True, 0.01),
    "512x384-d112-a32-b192": (512, 384, 112, 32, 192, True, 0.0),
    "768x256-d98-a23-b128": (768, 256, 98, 23, 128, False, 0.01),
    "1024x512-d67-a28-b256": (1024, 512, 67, 28, 256, True, 0.01),
    "256x128-d17-a2-b8256": (256, 128, 17, 2, 8256, True, 0.0),
}
SPLITK1 = "1024x512-d67-a28-b256"
ENTRIES = {"dm_ppo_wide_grad": ("DmPpoWideStep", "dm_ppo_wide_packed_elems", 1), "dm_ppo_wide3_grad": ("DmPpoWide3Step", "dm_ppo_wide3_packed_elems", 2)}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_case(_lib, entry, key, dev):
    step_cls, packed_elems, planes = ENTRIES[entry]
    H1, H2, D, A, B, normalize, ent = SHAPES[key]
    L = _lib.load_library()
    g = torch.Generator().manual_seed(1234)
    rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(dev)
    W = [[rnd(H1, D, scale=D ** -0.5), rnd(H2, H1, scale=H1 ** -0.5), rnd(At, H2, scale=0.1 * H2 ** -0.5)] for At in (A, 1)]
    b = [[rnd(H1, scale=0.1), rnd(H2, scale=0.1), rnd(At, scale=0.1)] for At in (A, 1)]
    log_std = rnd(A, scale=0.1)
    obs, act, adv, ret = rnd(B, D), rnd(B, A, scale=0.5), rnd(B), rnd(B)
    old_logp = (-0.5 * (act * torch.exp(-log_std)).pow(2).sum(1) - log_std.sum() - 0.9189385 * A + rnd(B, scale=0.05)).contiguous()
    n = sum(t.numel() for tr in W + b for t in tr) + A
    arena = torch.full((n,), float("nan"), device=dev)            # cleared by the fold
    gW, gb, off = [[None] * 3, [None] * 3], [[None] * 3, [None] * 3], 0
    for t in range(2):
        for l in range(3):
            gW[t][l] = arena[off:off + W[t][l].numel()]; off += W[t][l].numel()
            gb[t][l] = arena[off:off + b[t][l].numel()]; off += b[t][l].numel()
    g_log_std = arena[off:off + A]
    Dp = int(L.dm_ppo_wide_dp(D))
    bf = lambda e: torch.zeros(planes * e, dtype=torch.int16, device=dev)
    npk = int(getattr(L, packed_elems)(D, H1, H2)) // planes
    buf = {"xbT": bf((Dp + 31) // 32 * 32 * B)}
    for t in range(2):
        buf.update({"wpk%d" % t: bf(npk), "h1T%d" % t: bf(H1 * B), "dz1T%d" % t: bf(H1 * B), "h2T%d" % t: bf(H2 * B), "dz2T%d" % t: bf(H2 * B),
                    "dz3T%d" % t: bf(32 * B)})
    f32 = {"part": torch.zeros(2 * (B // 32) * 40, device=dev), "stats8": torch.zeros(8, device=dev), "out8": torch.zeros(8, device=dev)}
    state2, loss_acc = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    st = getattr(_lib, step_cls)()
    st.B, st.D, st.H1, st.H2, st.A = B, D, H1, H2, A
    st.normalize_advantage, st.clip_range, st.vf_coef, st.ent_coef = int(normalize), 0.2, 0.5, ent
    st.obs, st.act, st.adv, st.ret, st.old_logp = (t.data_ptr() for t in (obs, act, adv, ret, old_logp))
    st.log_std, st.g_log_std = log_std.data_ptr(), g_log_std.data_ptr()
    for t in range(2):
        for l in range(3):
            st.W[t][l], st.b[t][l], st.gW[t][l], st.gb[t][l] = (x[t][l].data_ptr() for x in (W, b, gW, gb))
        for k in ("wpk", "h1T", "dz1T", "h2T", "dz2T", "dz3T"):
            getattr(st, k)[t] = buf["%s%d" % (k, t)].data_ptr()
    st.xbT = buf["xbT"].data_ptr()
    st.part, st.stats8, st.out8 = (f32[k].data_ptr() for k in ("part", "stats8", "out8"))
    st.zero_ptr, st.zero_floats = arena.data_ptr(), n
    st.adam_state2, st.loss_acc = state2.data_ptr(), loss_acc.data_ptr()
    torch.cuda.synchronize()
    rc = getattr(L, entry)(C.byref(st), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if rc != 0:
        raise SystemExit("%s returned %d at %s" % (entry, rc, key))
    rec = {k: sha(v) for k, v in buf.items()}
    rec.update({k: sha(v) for k, v in f32.items()})
    rec["g_log_std"] = sha(g_log_std)
    rec["finite"] = bool(torch.isfinite(f32["out8"]).all()) and bool(torch.isfinite(arena).all())
    if key == SPLITK1:
        rec.update({"gW%d%d" % (t, l): sha(gW[t][l]) for t in range(2) for l in range(3)})
    return rec


def compare(a, b):
    A, B = (json.load(open(p))["cases"] for p in (a, b))
    differ = sorted("%s/%s" % (c, k) for c in set(A) | set(B) for k in set(A.get(c, {})) | set(B.get(c, {}))
                    if A.get(c, {}).get(k) != B.get(c, {}).get(k))
    print(json.dumps({"cases": [len(A), len(B)], "digests": sum(len(v) for v in A.values()), "differ": differ}, indent=1))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not torch.cuda.is_available():
        raise SystemExit("wide_digest.py runs the GPU kernels; no GPU is visible")
    import deepmimic_mujoco_amd._lib as _lib
    if os.environ.get("DM_LIB_VARIANT"):
        _lib.LIB_PATH = _lib.LIB_PATH.replace("libdeepmimic_hip.so", "libdeepmimic_hip_%s.so" % os.environ["DM_LIB_VARIANT"])
    dev = torch.device("cuda", 0)
    cases = {}
    for entry in ENTRIES:
        for key in SHAPES:
            cases["%s/%s" % (entry, key)] = run_case(_lib, entry, key, dev)
            print(json.dumps({"case": "%s/%s" % (entry, key), "finite": cases["%s/%s" % (entry, key)]["finite"]}), flush=True)
    out = {"workload": "wide_digest", "device": torch.cuda.get_device_name(0), "cases": cases}
    print(json.dumps({"workload": "wide_digest", "cases": len(cases), "digests": sum(len(v) for v in cases.values())}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
