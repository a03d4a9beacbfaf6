"""What the GPU tests of the learner kernels share: library / pointer / stream accessors, NaN-guarded output buffers, offset input
views, the measured-against-bound print, the element-by-element `within` check, the out8 check and the Python restatement of the kernels' counter-based draws
(csrc/dm_rng.h).  A plain module: importing it touches no GPU."""
import ctypes as C
import functools

import numpy as np
import torch

DEV = torch.device("cuda", 0)
GUARD = 4096             # NaN floats / 0x7FC0 bf16 behind every guarded array: a stray write shows up there
BF16_NAN = 0x7FC0


def lib():
    from deepmimic_mujoco_amd import _lib as L
    return L.load_library()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device=DEV):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def guarded(*shape, fill=float("nan")):
    """(buffer, view): an fp32 buffer and a contiguous view of `shape` at its start, filled with `fill`; GUARD floats of NaN behind
    the view."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), device=DEV)
    if fill == fill:
        buf[:n] = fill
    return buf, buf[:n].view(*shape)


def guard_ok(buf, view):
    return bool(torch.isnan(buf[view.numel():]).all())


def guarded_bf16(n):
    """(buffer, view) of bf16 scratch as int16, every element 0x7FC0 (a bf16 NaN), GUARD elements behind the view."""
    buf = torch.full((n + GUARD,), BF16_NAN, dtype=torch.int16, device=DEV)
    return buf, buf[:n]


def guard_ok_bf16(buf, view):
    return bool((buf[view.numel():] == BF16_NAN).all())


def offset(t, off):
    """The same values as a view that starts `off` elements into a larger buffer."""
    buf = torch.zeros(t.numel() + off + 7, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def note(what, err, tol, width=34):
    """The measured error against its bound (printed with pytest -s: the numbers the docstrings quote)."""
    print("measured %-*s %10.3g   bound %10.3g   margin %8.1fx" % (width, what, err, tol, tol / max(err, 1e-30)))
    return err


MISSES = []


def checked(test):
    """`within` records a miss and goes on, so one run shows every quantity that is out of bounds; the test fails at its end."""
    @functools.wraps(test)
    def run(*args, **kw):
        MISSES.clear()
        test(*args, **kw)
        assert not MISSES, MISSES
    return run


def within(what, got, val, bnd):
    """Every element of `got` within its bound of the fp64 value; prints the worst error / bound (a NaN or an error against a zero
    bound is a miss)."""
    g = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    val = np.asarray(val, np.float64)
    g = g.reshape(val.shape)
    err = np.abs(g - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / np.broadcast_to(np.asarray(bnd, np.float64), val.shape))
    worst = float(np.max(ratio)) if ratio.size else 0.0
    note(what, worst, 1.0, width=46)
    if not worst <= 1.0:
        MISSES.append((what, round(worst, 2), "element %d, %d of %d out" % (int(np.argmax(ratio)), int((~(ratio <= 1.0)).sum()), ratio.size)))
    return worst


def check_out8(out8, ref8, ratio64, clip, B, width=34):
    """loss terms within 2e-5 x max(1, |ref|) (the A = 28 loss bound), approx_kl within 5e-5, the advantage statistics within
    1e-5 relative, the clip fraction exact up to the samples whose fp64 ratio lies within 1e-3 of the clip boundary."""
    o, r = [float(x) for x in out8], [float(x) for x in ref8]
    for k in (0, 1, 2, 3):
        assert note("out8[%d]" % k, abs(o[k] - r[k]), 2e-5 * max(1.0, abs(r[k])), width) < 2e-5 * max(1.0, abs(r[k])), (k, o[k], r[k])
    assert note("out8[4] approx_kl", abs(o[4] - r[4]), 5e-5, width) < 5e-5, (o[4], r[4])
    amb = int((((ratio64 - 1).abs() - clip).abs() < 1e-3).sum())
    assert abs(o[5] - r[5]) <= amb / B + 1e-6, (o[5], r[5], amb)
    assert abs(o[6] - r[6]) < 1e-5 * max(1.0, abs(r[6])) and abs(o[7] - r[7]) < 1e-5 * abs(r[7])


def hash32(seed, a, b, c):
    """dm_hash32 of csrc/dm_rng.h (the step kernels and the oracle use the same mix): wrapping uint64 arithmetic, broadcast over
    integer arrays; a Python int when every argument is a scalar."""
    u = lambda v: np.asarray(v).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = u(seed) ^ (u(a) * np.uint64(0x9E3779B97F4A7C15)) ^ (u(b) * np.uint64(0xBF58476D1CE4E5B9)) ^ (u(c) * np.uint64(0x94D049BB133111EB))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = (x ^ (x >> np.uint64(31))) >> np.uint64(32)
    return int(x) if x.ndim == 0 else x


def normals(seed, rows, ctr, A):
    """dm_normal2 in float64, eps [rows x A]: the Box-Muller pair (j, j + 1) of (seed, row, ctr) from the uniforms of hashes j
    (in (0, 1]) and j + 1 (in [0, 1)), cosine first; the last pair of an odd A is half used."""
    r = np.arange(rows)[:, None]
    j = np.arange(0, A + 1, 2)[None, :]
    u1 = ((hash32(seed, r, ctr, j) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (hash32(seed, r, ctr, j + 1) >> np.uint64(8)).astype(np.float64) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], -1).reshape(rows, -1)[:, :A]
