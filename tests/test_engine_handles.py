"""The lifetime of the engine's handle classes and of its named device buffers, against a stub in place of the library:
no GPU, and libvoxelhashing_amd.so is never loaded."""
import ctypes as C
import sys
import types

import numpy as np
import pytest

from voxelhashing_amd import engine as E
from voxelhashing_amd import lib
from voxelhashing_amd import vhtypes as T
from voxelhashing_amd.engine import _common


class StubLib:
    """every vh_* symbol: records its name and arguments, hands out handles and device pointers, returns 0"""

    def __init__(self, create_code=0, destroy_raises=False):
        self.create_code, self.destroy_raises = create_code, destroy_raises
        self.calls, self.freed, self.uploads = [], [], []
        self._next = 0x1000

    def names(self, suffix=""):
        return [name for name, _ in self.calls if name.endswith(suffix)]

    def _fresh(self):
        self._next += 0x100
        return self._next

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name == "vh_error_string":
                return b"stub error"
            if name == "vh_last_error_message":
                return b""
            if name.endswith("_create"):
                if self.create_code == 0:
                    args[-1]._obj.value = self._fresh()
                return self.create_code
            if name.endswith("_destroy"):
                if self.destroy_raises:
                    raise RuntimeError("destroy failed")
                return None
            if name == "vh_malloc":
                args[0]._obj.value = self._fresh()
            if name == "vh_free":
                self.freed.append(args[0])
            if name == "vh_memcpy_h2d":
                self.uploads.append((args[0], bytes((C.c_char * args[2]).from_address(args[1]))))
            if name == "vh_hash_data_alloc":
                args[0]._obj.d_hash = self._fresh()
            return 0
        return fn


@pytest.fixture
def stub(monkeypatch):
    def install(**kw):
        s = StubLib(**kw)
        for mod in [lib] + [m for name, m in sys.modules.items() if name.startswith(E.__name__ + ".") and isinstance(m, types.ModuleType)]:
            if hasattr(mod, "load"):
                monkeypatch.setattr(mod, "load", lambda: s)
        return s
    return install


def _scene():
    return types.SimpleNamespace(handle=C.c_void_p(0x10))


HANDLE_CLASSES = {
    "CUDASceneRepHashSDF": lambda: E.CUDASceneRepHashSDF(T.HashParams()),
    "CUDARayCastSDF": lambda: E.CUDARayCastSDF(T.RayCastParams()),
    "CUDASceneRepChunkGrid": lambda: E.CUDASceneRepChunkGrid(_scene(), (1.0, 1.0, 1.0), (4, 4, 4), (-2, -2, -2), 16, True, 2),
    "Reconstruction": lambda: E.Reconstruction(_scene(), None, None, T.DepthCameraParams()),
    "CUDAMarchingCubesHashSDF": lambda: E.CUDAMarchingCubesHashSDF(T.MarchingCubesParams()),
    "CUDARGBDSensor": lambda: E.CUDARGBDSensor((64, 48), (64, 48), (32, 24), 50.0, 50.0, 16.0, 12.0, 0.1, 4.0),
    "CUDACameraTrackingMultiRes": lambda: E.CUDACameraTrackingMultiRes(32, 24, 3),
    "CUDACameraTrackingMultiResRGBD": lambda: E.CUDACameraTrackingMultiResRGBD(32, 24, 3),
    "RGBDRenderer": lambda: E.RGBDRenderer(),
    "PhongLighting": lambda: E.PhongLighting(T.PhongLight()),
}


def test_every_class_with_a_handle_is_listed_and_takes_its_lifetime_from_the_base():
    with_handle = {name for name, obj in vars(E).items() if isinstance(obj, type) and issubclass(obj, _common._Handle) and obj._destroy}
    assert with_handle == set(HANDLE_CLASSES)
    for name in with_handle:
        own = vars(getattr(E, name))
        assert "close" not in own and "__del__" not in own and own["_destroy"].endswith("_destroy")
    for cls in (E.LauncherScene, E.LiveMesh):  # own structs, no handle: their own close(), the base's __del__
        assert issubclass(cls, _common._Handle) and "close" in vars(cls) and "__del__" not in vars(cls)


@pytest.mark.parametrize("name", sorted(HANDLE_CLASSES))
def test_close_twice_destroys_once(stub, name):
    s = stub()
    obj = HANDLE_CLASSES[name]()
    assert obj.L is s and len(s.names("_create")) == 1 and obj.handle.value == s._next
    handle = obj.handle
    obj.close()
    obj.close()
    obj.__del__()
    destroyed = [(n, a) for n, a in s.calls if n.endswith("_destroy")]
    assert [n for n, _ in destroyed] == [type(obj)._destroy] and destroyed[0][1] == (handle,)
    assert obj.handle is None


@pytest.mark.parametrize("name", sorted(HANDLE_CLASSES))
def test_a_failed_create_raises_and_leaves_nothing_to_destroy(stub, name, monkeypatch):
    s = stub(create_code=4)
    made = []
    base_create = _common._Handle._create
    monkeypatch.setattr(_common._Handle, "_create", lambda self, *a: (made.append(self), base_create(self, *a)))
    with pytest.raises(E.VhError) as e:
        HANDLE_CLASSES[name]()
    assert e.value.code == 4 and "_create: stub error (code 4)" in str(e.value)
    obj, = made
    assert not obj.handle
    obj.close()
    obj.__del__()
    assert s.names("_destroy") == []


def test_del_swallows_what_destroy_raises_and_close_does_not(stub):
    s = stub(destroy_raises=True)
    obj = E.RGBDRenderer()
    obj.__del__()
    assert s.names("_destroy") == ["vh_rgbd_renderer_destroy"]
    with pytest.raises(RuntimeError, match="destroy failed"):
        obj.close()


def test_launcher_scene_synchronizes_its_stream_before_it_frees(stub):
    s = stub()
    stream = C.c_void_p(0x77)
    g = E.LauncherScene(T.HashParams(), stream=stream)
    del s.calls[:]
    g.close()
    assert [n for n, _ in s.calls] == ["vh_stream_synchronize", "vh_hash_data_free"] and s.calls[0][1] == (stream,)


def test_live_mesh_close_frees_once(stub):
    s = stub()
    m = E.LiveMesh(T.MarchingCubesParams(), 8)
    m.close()
    m.close()
    m.__del__()
    assert s.names("_free") == ["vh_live_mesh_data_free", "vh_marching_cubes_data_free", "vh_free"]


def test_buffers_are_freed_once_each_when_the_body_raises(stub):
    s = stub()
    with pytest.raises(ZeroDivisionError):
        with _common._Buffers(stream=None) as bufs:
            a = bufs.upload("a", np.arange(5, dtype=np.uint32))
            b = bufs.alloc("b", 64)
            c = bufs.alloc("c", 12, fill=0xa5a5a5a5)
            ptrs = [a.ptr, b.ptr, c.ptr]
            assert bufs["b"] is b and len(set(ptrs)) == 3
            assert s.uploads == [(a.ptr, np.arange(5, dtype=np.uint32).tobytes()), (c.ptr, b"\xa5" * 12)]
            1 / 0
    assert sorted(s.freed) == sorted(ptrs)
    for buf in (a, b, c):
        buf.free()  # (and their __del__ later)
    assert sorted(s.freed) == sorted(ptrs)


def test_buffers_download_by_name_and_refuse_a_name_twice(stub):
    s = stub()
    with _common._Buffers(stream=None) as bufs:
        bufs.alloc("x", 16)
        assert bufs.download("x", np.uint32).shape == (4,) and s.names("vh_memcpy_d2h") == ["vh_memcpy_d2h"]
        with pytest.raises(KeyError):
            bufs.alloc("x", 16)
        with pytest.raises(KeyError):
            bufs["y"]
    assert len(s.freed) == 2 and len(set(s.freed)) == 2  # x, and the second buffer that found the name taken
