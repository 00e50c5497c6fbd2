"""Test helper: the entry-record builder on the host (cuda-raytracing_amd/librt_entry_host.so, csrc/entry_host.h), built
by build() beside the product library and kept out of its ABI."""
import ctypes
import os

import rt_testlib as T

rt = T.load_rt()
_P, _I, _SZ, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint64
_L = None


def _lib():
    global _L
    if _L is None:
        rt.lib()  # librt_hip.so first: the helper links against it
        L = ctypes.CDLL(os.path.join(rt.PKG_DIR, "librt_entry_host.so"))
        for name, (res, args) in {
                "rt_entry_host_create": (_P, []),
                "rt_entry_host_destroy": (None, [_P]),
                "rt_entry_host_update": (_I, [_P, _P, _SZ, _P, _SZ, _P, _SZ, _P, _SZ, _P, _I, _I]),
                "rt_entry_host_builds": (_U64, [_P]),
                "rt_entry_host_records": (_P, [_P, ctypes.POINTER(_SZ)]),
                "rt_entry_host_nodes": (_P, [_P, ctypes.POINTER(_SZ)]),
                "rt_entry_host_dropped": (_I, [_P, _I, _I, _P, _I]),
                "rt_entry_host_replay": (_I, [_P, _SZ, _P, _P, _P, _P, _P])}.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _L = L
    return _L


class EntryReplay(ctypes.Structure):
    """rt_entry_replay (rt_abi.h)."""
    _fields_ = [("face_root", ctypes.c_uint32), ("face_entry", ctypes.c_uint32), ("t_root", ctypes.c_float),
                ("t_entry", ctypes.c_float), ("visits_root", ctypes.c_uint32), ("visits_entry", ctypes.c_uint32),
                ("qualifies", ctypes.c_int32), ("dropped_hit", ctypes.c_int32), ("direction", ctypes.c_float * 3),
                ("stack_root", ctypes.c_uint32), ("stack_entry", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class EntryHost:
    """The camera rays' entry table on the host (rt_entry_host_*, csrc/entry_frontier.h): the device builder's code
    and rt_render's key rule over a scene's host arrays, for the tests."""

    def __init__(self):
        self.handle = _lib().rt_entry_host_create()
        self._keep = None

    def __del__(self):
        if getattr(self, "handle", None):
            _lib().rt_entry_host_destroy(self.handle)
            self.handle = None

    def update(self, arrays, camera, width, height):
        """`arrays`: Scene.host_arrays() (kept alive here: the node array's address is part of the key); returns
        True when the table was rebuilt."""
        import numpy as np
        if self._keep is None or self._keep[0] is not arrays:
            self._keep = (arrays, {k: np.ascontiguousarray(v) for k, v in arrays.items()})
        a = self._keep[1]
        cam = camera if isinstance(camera, rt.GPUCamera) else rt.GPUCamera.from_buffer_copy(np.asarray(camera, np.float32).tobytes())
        rc = _lib().rt_entry_host_update(self.handle, a["nodes"].ctypes.data, a["nodes"].size // 32, a["face_indices"].ctypes.data,
                                        a["face_indices"].size // 4, a["faces"].ctypes.data, a["faces"].size // 16,
                                        a["vertices"].ctypes.data, a["vertices"].size // 32, ctypes.byref(cam), int(width),
                                        int(height))
        if rc < 0:
            raise rt.RTError("rt_entry_host_update: " + rt.lib().rt_last_error().decode())
        return rc == 1

    @property
    def builds(self):
        return int(_lib().rt_entry_host_builds(self.handle))

    def records(self):
        """(tiles, 16) uint32: count, then node indices in visit order."""
        import numpy as np
        n = ctypes.c_size_t()
        p = _lib().rt_entry_host_records(self.handle, ctypes.byref(n))
        return np.frombuffer(ctypes.string_at(p, n.value * 64), dtype=np.uint32).reshape(-1, 16).copy()

    def nodes(self):
        """The private node array the records index, (N, 8) float32."""
        import numpy as np
        n = ctypes.c_size_t()
        p = _lib().rt_entry_host_nodes(self.handle, ctypes.byref(n))
        return np.frombuffer(ctypes.string_at(p, n.value * 32), dtype=np.float32).reshape(-1, 8).copy()

    def dropped(self, tile_x, tile_y):
        import numpy as np
        out = np.zeros(4096, dtype=np.uint32)
        n = _lib().rt_entry_host_dropped(self.handle, int(tile_x), int(tile_y), out.ctypes.data, out.size)
        if n < 0 or n > out.size:
            raise rt.RTError("rt_entry_host_dropped: no such sub-tile")
        return out[:n]

    def replay(self, px, py, ru, rv):
        """The reference's walk of the camera rays (pixel, jitter) from the root and from their records: a numpy
        record array with EntryReplay's fields."""
        import numpy as np
        px, py = np.ascontiguousarray(px, dtype=np.int32), np.ascontiguousarray(py, dtype=np.int32)
        ru, rv = np.ascontiguousarray(ru, dtype=np.float32), np.ascontiguousarray(rv, dtype=np.float32)
        out = np.zeros(px.size, dtype=np.dtype(EntryReplay))
        if _lib().rt_entry_host_replay(self.handle, px.size, px.ctypes.data, py.ctypes.data, ru.ctypes.data, rv.ctypes.data,
                                       out.ctypes.data) != 0:
            raise rt.RTError("rt_entry_host_replay: " + rt.lib().rt_last_error().decode())
        return out
