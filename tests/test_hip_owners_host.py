"""The owners of one argument shape each in hip.py, called as plain functions of (array, dims) without a context
(tests/test_hip_binding_host.py states what the methods built on them hand to the library)."""
import ctypes as C

import numpy as np
import pytest


def test_batch_promotes_one_column_and_checks_the_rest(hank):
    from hank_amd.hip import _batch
    x = np.arange(6.0).reshape(2, 3)
    a, N = _batch(x, (2, 3))
    assert N == 1 and a.shape == (2, 3, 1) and a.flags.f_contiguous and np.array_equal(a[:, :, 0], x)
    b = np.arange(24.0).reshape(2, 3, 4)
    a, N = _batch(b, (2, 3))
    assert N == 4 and a.strides == (8, 16, 48) and np.array_equal(a, b)
    assert _batch(x, (2, 3), N=1)[1] == 1
    with pytest.raises(ValueError, match=r"expected array of shape \(2, 3, 4\), got \(2, 3, 1\)"):
        _batch(x, (2, 3), N=4)                                    # a given N is checked, not taken from x
    with pytest.raises(ValueError, match=r"expected array of shape \(3, 2, 4\), got \(2, 3, 4\)"):
        _batch(b, (3, 2))
    with pytest.raises(ValueError, match=r"expected array of shape \(2, 3, 0\), got \(2,\)"):
        _batch(np.zeros(2), (2, 3), strict=True)                  # strict: a wrong rank is a batch of no columns
    assert _batch(np.zeros((2, 3, 0)), (2, 3), strict=True)[1] == 0


def test_seeds_take_one_width_and_name_what_is_missing(hank):
    from hank_amd.hip import _seeds
    u, v = np.ones((2, 3)), np.ones((5, 4))
    N, (a, b, c) = _seeds((("u", u, (2,)), ("v", None, (5,)), ("w", v, lambda s, N: ("w", s.shape, N))))
    assert N == 3 and a.shape == (2, 3) and b is None and c == ("w", (5, 4), 3)
    N, (a, b) = _seeds((("u", None, (2,)), ("v", v[:, 0], (5,))))
    assert N == 1 and a is None and b.shape == (5, 1)
    assert _seeds((("u", u[:, :1], (2,)),), N=1)[0] == 1
    with pytest.raises(ValueError, match="^at least one of u, v must be given$"):
        _seeds((("u", None, (2,)), ("v", None, (5,))))
    with pytest.raises(ValueError, match=r"expected array of shape \(5, 3\), got \(5, 4\)"):
        _seeds((("u", u, (2,)), ("v", v, (5,))))
    bad = (("u", np.ones((7, 3)), (2,)), ("v", v, (5,)))
    with pytest.raises(ValueError, match=r"expected array of shape \(2, 3\), got \(7, 3\)"):
        _seeds(bad)
    with pytest.raises(ValueError, match=r"expected array of shape \(5, 3\), got \(5, 4\)"):
        _seeds(bad, last_first=True)


def test_grid_batches_outputs_counts_and_device_pointers(hank):
    from hank_amd.hip import _dev, _grid_batch, _n1, _out
    m = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(_grid_batch(m, 4, 3), m.reshape((12, 1), order="F"))
    b = np.arange(24.0).reshape(4, 3, 2)
    assert np.array_equal(_grid_batch(b, 4, 3)[:, 1], b[:, :, 1].reshape(-1, order="F"))
    for other in (np.zeros((12, 2)), np.zeros(12), np.zeros((3, 4, 2))):
        assert _grid_batch(other, 4, 3).shape == other.shape
    assert [_n1(n) for n in (-1, 0, 1, 3, np.int64(5))] == [1, 1, 1, 3, 5] and type(_n1(np.int64(5))) is int
    o = _out(2, 3, 4)
    assert o.shape == (2, 3, 4) and o.dtype == np.float64 and o.strides == (8, 16, 48)
    assert _out(5, 0).shape == (5, 0)
    assert _dev(0).value is None and _dev(None).value is None and _dev(4096).value == 4096 and isinstance(_dev(0), C.c_void_p)


def test_a_status_is_raised_from_the_context_or_from_a_message(hank):
    from hank_amd import hip

    class Lib:
        def hank_last_error(self, ctx):
            return b"from the context"

    assert hip._raise_status(Lib(), None, hip.HANK_OK) is None
    with pytest.raises(hip.DomainError, match=r"^\[hank_hip status 4\] from the context$"):
        hip._raise_status(Lib(), None, hip.HANK_ERR_DOMAIN)
    with pytest.raises(hip.NoDeviceError, match=r"^\[hank_hip status 1\] given$"):
        hip._raise_status(None, None, hip.HANK_ERR_NO_DEVICE, "given")
