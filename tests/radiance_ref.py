"""Plain-numpy helpers for the rt_radiance tests (tests/test_radiance_cpu.py, tests/test_gpu_radiance.py).

The yardstick is the oracle's oracle_sample_table (oracle/rt_oracle.c): for a pixel and an RNG state, the colour and
the number of draws of one camera sample started at every even draw offset.  A caller-given ray that is the jittered
camera ray of draws (2i, 2i + 1), handed the state advanced by 2i + 2, must therefore get table row i bit for bit and
leave the state advanced by 2i + draws_i.  What is restated here is only what surrounds that table: the XORWOW step
(rng_next, checked against oracle_rng_draws by the CPU tests), curand_uniform, and the camera-ray arithmetic of the
sample start (checked through the table chain against oracle_render).
"""
import ctypes

import numpy as np

import rt_testlib as T

F32, U32 = np.float32, np.uint32
STATE_WORDS = 12  # rt_rng_state: d, v[5], six unused words


def xorwow_step(states):
    """One rng_next on every row of a uint32 [N, 6] array (d, v0..v4), in place; returns the draws (uint32 [N])."""
    d, v = states[:, 0], states[:, 1:]
    t = v[:, 0] ^ (v[:, 0] >> U32(2))
    new4 = (v[:, 4] ^ (v[:, 4] << U32(4))) ^ (t ^ (t << U32(1)))
    v[:, 0:4] = v[:, 1:5].copy()
    v[:, 4] = new4
    d += U32(362437)
    return v[:, 4] + d


def xorwow_advance(states, n):
    """A copy of the uint32 [N, 6] states advanced by n draws; n an int or an integer array [N] (per row)."""
    out = np.array(states, dtype=U32, copy=True).reshape(-1, 6)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (out.shape[0],))
    assert (n >= 0).all()
    for k in range(int(n.max()) if n.size else 0):
        rows = np.flatnonzero(n > k)
        sub = out[rows]
        xorwow_step(sub)
        out[rows] = sub
    return out


def uniforms(states, n):
    """The next n curand_uniform draws of every state, float32 [N, n] (the states are not changed):
    (float)x * 2^-32 + 2^-33 in fp32."""
    s = np.array(states, dtype=U32, copy=True).reshape(-1, 6)
    out = np.zeros((s.shape[0], n), dtype=F32)
    for k in range(n):
        out[:, k] = xorwow_step(s).astype(F32) * F32(2.0 ** -32) + F32(2.0 ** -33)
    return out


def jittered_camera_rays(camera15, w, h, ru, rv):
    """rt_ray rows [h * w, 8] of the renderer's camera sample for jitter (ru, rv) (float32 [h * w], pixel y * w + x):
    ux = (float32(x) + ru) / float32(w), uy likewise, rd = ((cl + ch * ux) + cv * uy) - co, ro = co -- fp32, in that
    order, nothing fused.  tmax = 1e30."""
    cam = np.asarray(camera15, dtype=F32)
    co, ch, cv, cl = cam[0:3], cam[6:9], cam[9:12], cam[12:15]
    x = np.tile(np.arange(w), h).astype(F32)
    y = np.repeat(np.arange(h), w).astype(F32)
    ux = ((x + np.asarray(ru, dtype=F32)) / F32(w)).astype(F32)
    uy = ((y + np.asarray(rv, dtype=F32)) / F32(h)).astype(F32)
    rays = np.zeros((w * h, 8), dtype=F32)
    for k in range(3):
        a = (ch[k] * ux).astype(F32)
        b = (cv[k] * uy).astype(F32)
        rays[:, 4 + k] = (((cl[k] + a).astype(F32) + b).astype(F32) - co[k]).astype(F32)
        rays[:, k] = co[k]
    rays[:, 3] = F32(1e30)
    return rays


_table_fn = None


def sample_table(oracle_scene, w, h, x, y, bounces, state, n):
    """oracle_sample_table for pixel (x, y): float32 [n, 8] rows (r, g, b, draws, segments, nodes, tris, 0)."""
    global _table_fn
    if _table_fn is None:
        fn = T.oracle().oracle_sample_table
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        _table_fn = fn
    st = np.ascontiguousarray(state, dtype=U32)
    out = np.zeros((n, 8), dtype=F32)
    assert _table_fn(oracle_scene.h, w, h, x, y, bounces, st.ctypes.data, n, out.ctypes.data) == 0
    return out


_TABLES = {}


def frame_tables(key, oracle_scene, w, h, bounces, states, n):
    """sample_table of every pixel of a frame, float32 [h * w, n, 8]; computed once per (key, n) and shared (never
    modified by a test)."""
    got = _TABLES.get((key, n))
    if got is None:
        got = np.stack([sample_table(oracle_scene, w, h, p % w, p // w, bounces, states[p], n) for p in range(w * h)])
        got.setflags(write=False)
        _TABLES[(key, n)] = got
    return got


def chain_frame(tables, spp):
    """Frame 0 of oracle_render from the tables ([P, n, 8]): per pixel, follow the sample chain o_0 = 0,
    o_{j+1} = o_j + draws(o_j) through the table (entry o / 2) and average `spp` samples as the renderer does.
    Returns (rgba float32 [P, 4], draws consumed int64 [P])."""
    P, n, _ = tables.shape
    acc = np.zeros((P, 3), dtype=F32)
    off = np.zeros(P, dtype=np.int64)
    rows = np.arange(P)
    for _ in range(spp):
        assert (off % 2 == 0).all() and (off // 2 < n).all(), "the table is too short for the chain"
        row = tables[rows, off // 2]
        acc = (acc + row[:, 0:3]).astype(F32)
        off = off + row[:, 3].astype(np.int64)
    out = np.ones((P, 4), dtype=F32)
    out[:, 0:3] = (acc / F32(spp)).astype(F32)
    return out, off


def pack_states(states6):
    """uint32 [N, 6] states as the int32 [N * 12] words of rt_rng_state rows (the unused words zero)."""
    s = np.asarray(states6, dtype=U32).reshape(-1, 6)
    out = np.zeros((s.shape[0], STATE_WORDS), dtype=U32)
    out[:, :6] = s
    return out.reshape(-1).view(np.int32)
