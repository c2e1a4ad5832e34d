"""The numpy side of the env shims' array backend (_arrays.py): the device parser, buffer dtypes, action / mask
conversion and the block checks with their ValueErrors.  No GPU: the torch side runs in test_gpu_shim_paths.py."""
import numpy as np
import pytest

from underwater_swimmer_rl_amd import _capi
from underwater_swimmer_rl_amd._arrays import ArrayBackend, device_index


@pytest.fixture
def host():
    b = ArrayBackend()
    b._init_arrays("numpy", 0)
    return b


def test_device_index():
    assert [device_index(d) for d in ("cuda:3", 3, "cuda", "cuda:0", 0, np.int64(2))] == [3, 3, 0, 0, 0, 2]


def test_a_numpy_backend_passes_host_pointers_on_the_null_stream(host):
    assert host._torch is None and host.device is None
    assert host._flags == 0 and _capi.SALP_DEVICE_PTRS == 1 and host._stream == 0


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int32, np.float64, np.bool_])
def test_empty_dtypes(host, dtype):
    a = host._empty((5, 3), dtype)
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (5, 3) and a.flags.c_contiguous


def test_actions_in(host):
    want = np.linspace(-1, 1, 12, dtype=np.float32).reshape(6, 2)
    strided = np.zeros((6, 4))
    strided[:, ::2] = want
    for given in (want.tolist(), want.astype(np.float64), strided[:, ::2], want.reshape(12), want):
        a = host._actions_in(given, (6, 2))
        assert a.dtype == np.float32 and a.shape == (6, 2) and a.flags.c_contiguous and np.array_equal(a, want)
    assert host._actions_in(np.arange(24.0), (3, 4, 2)).shape == (3, 4, 2)
    with pytest.raises(ValueError):
        host._actions_in(np.zeros(11), (6, 2))


def test_mask_in(host):
    want = np.array([1, 0, 0, 1, 1, 0], np.uint8)
    for given in ([True, False, False, True, True, False], want.astype(np.bool_), want.astype(np.float64), want,
                  np.repeat(want, 2)[::2]):
        m = host._mask_in(given)
        assert m.dtype == np.uint8 and m.shape == (6,) and m.flags.c_contiguous and np.array_equal(m, want)
    assert host._mask_in(None) is None


def test_bool_view_shares_the_bytes(host):
    b = np.array([0, 1, 1, 0], np.uint8)
    v = host._bool_view(b)
    assert v.dtype == np.bool_ and v.tolist() == [False, True, True, False]
    b[0] = 1
    assert v[0] and np.shares_memory(v, b)


def test_is_block(host):
    good = np.zeros((4, 3, 2), np.float64)
    assert host._is_block(good, (4, 3, 2), np.float64) and host._is_block(good, [4, 3, 2], np.float64)
    assert not host._is_block(good, (4, 3, 2), np.float32)                               # dtype
    assert not host._is_block(good, (4, 6), np.float64)                                  # shape
    assert not host._is_block(np.zeros((4, 3, 4))[:, :, ::2], (4, 3, 2), np.float64)     # contiguity
    assert not host._is_block(good.tolist(), (4, 3, 2), np.float64)                      # not an array
    assert not host._is_block(None, (4, 3, 2), np.float64)


def test_out_block(host):
    new = host._out_block(None, (7, 8), np.int32)
    assert new.dtype == np.int32 and new.shape == (7, 8)
    mine = np.zeros((7, 8), np.int32)
    assert host._out_block(mine, (7, 8), np.int32) is mine
    with pytest.raises(ValueError, match=r"^out must be an int32 \[7, 8\] block$"):
        host._out_block(np.zeros((7, 20), np.int32), (7, 8), np.int32)
    with pytest.raises(ValueError, match=r"^out must be an int32 \[7, 20\] block$"):
        host._out_block(np.zeros((8, 20), np.int32), (7, 20), np.int32)
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=r"^out must be a numpy array \(this env returns host arrays\)$"):
        host._out_block(torch.zeros((7, 8), dtype=torch.int32), (7, 8), np.int32)
    with pytest.raises(ValueError, match=r"^out must be a numpy array \(this env returns host arrays\)$"):
        host._out_block([[0] * 8] * 7, (7, 8), np.int32)


def test_the_call_helper_passes_addresses_and_raises_the_librarys_message():
    """`_capi.address` / `_capi.call` on a stand-in library: arrays by address, everything else as it is, and a nonzero
    status raised with the message of the header the symbol belongs to."""
    a = np.zeros(3, np.float32)
    assert _capi.address(a) == a.ctypes.data and _capi.address(None) is None and _capi.address(12) == 12
    assert _capi.SalpLib._ptr(a) == a.ctypes.data

    class Lib:
        seen = None

        def ok(self, *args):
            Lib.seen = args
            return 0

        salp_vec_fails = salp_robot_vec_fails = staticmethod(lambda *args: -1)
        salp_last_error = staticmethod(lambda: b"snake message")
        salp_robot_last_error = staticmethod(lambda: b"robot message")

    _capi.call(Lib(), "ok", a, None, 5, 2.5)
    assert Lib.seen == (a.ctypes.data, None, 5, 2.5)
    with pytest.raises(_capi.SalpError, match=r"^salp_vec_fails failed \(-1\): snake message$"):
        _capi.call(Lib(), "salp_vec_fails")
    with pytest.raises(_capi.SalpError, match=r"^step failed \(-1\): robot message$"):
        _capi.call(Lib(), "salp_robot_vec_fails", what="step")
