"""CPU checks of the Python boundary to libgpk: `Backend.call` / `Backend.status` on a shell object (no GPU: the handle,
the library and the stream binding are fakes), the two pointer converters of `_lib`, and a source check that the package
enters the library nowhere else."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

from conftest import ROOT


class _FakeLib:
    """Stands in for the loaded library: every `gpk_*` attribute is a function that records its call and returns the next
    status queued for it (default GPK_OK)."""

    def __init__(self, log, lock):
        self.log, self.lock, self.rc, self.held = log, lock, {}, []

    def gpk_last_error(self, h):
        return b"the library's own words"

    def __getattr__(self, name):
        if not name.startswith("gpk_"):
            raise AttributeError(name)

        def fn(*args):
            self.log.append((name, args))
            # the lock is held by this thread during the call: another thread cannot take it
            got = []
            t = threading.Thread(target=lambda: got.append(self.lock.acquire(blocking=False)))
            t.start()
            t.join()
            self.held.append(not got[0])
            return self.rc.get(name, 0)

        return fn


@pytest.fixture
def shell():
    from unmanned_aerial_vehicles_amd.device import Backend
    be = Backend.__new__(Backend)
    be.log = []
    be.lock = threading.RLock()
    be.lib = _FakeLib(be.log, be.lock)
    be.h = ctypes.c_void_p(0x1234)
    be.bind_stream = lambda: be.log.append(("bind", ()))
    return be


def test_call_binds_then_calls_with_the_handle_first_under_the_lock(shell):
    be = shell
    assert be.call("gpk_gram", 1, 2.5, None) == 0
    assert be.log == [("bind", ()), ("gpk_gram", (be.h, 1, 2.5, None))]
    assert be.lib.held == [True]
    # afterwards the lock is free again, and an outer `with be.lock` can be re-entered by call
    assert be.lock.acquire(blocking=False)
    be.lock.release()
    with be.lock:
        be.call("gpk_wtw", 7)
        be.call("gpk_lml_grad", 8)
    assert be.log[2:] == [("bind", ()), ("gpk_wtw", (be.h, 7)), ("bind", ()), ("gpk_lml_grad", (be.h, 8))]
    assert be.lib.held == [True, True, True]
    assert be.lock.acquire(blocking=False)
    be.lock.release()


def test_call_raises_what_check_raises(shell):
    from unmanned_aerial_vehicles_amd._lib import GPK_BAD_ARG, GPK_HIP_ERROR, GPK_NOT_PD, GPKError, NotPositiveDefinite
    be = shell
    be.lib.rc["gpk_potrf"] = GPK_NOT_PD
    with pytest.raises(NotPositiveDefinite, match="the library's own words"):
        be.call("gpk_potrf", 1)
    assert issubclass(NotPositiveDefinite, np.linalg.LinAlgError)
    for code in (GPK_BAD_ARG, GPK_HIP_ERROR):
        be.lib.rc["gpk_potrs"] = code
        with pytest.raises(GPKError, match="the library's own words") as e:
            be.call("gpk_potrs", 1)
        assert e.value.code == code
    # a failed call leaves the lock free
    assert be.lock.acquire(blocking=False)
    be.lock.release()


def test_status_returns_the_code_unchecked_and_still_binds(shell):
    from unmanned_aerial_vehicles_amd._lib import GPK_NOT_PD
    be = shell
    be.lib.rc["gpk_sparse_eval"] = GPK_NOT_PD
    assert be.status("gpk_sparse_eval", 3) == GPK_NOT_PD
    assert be.status("gpk_batch_end") == 0
    assert be.log == [("bind", ()), ("gpk_sparse_eval", (be.h, 3)), ("bind", ()), ("gpk_batch_end", (be.h,))]
    assert be.lib.held == [True, True]


def test_close_destroys_the_handle_once(shell):
    be = shell
    h = be.h
    be.close()
    be.close()
    assert be.h is None and be.log == [("gpk_destroy", (h,))]


def test_host_pointer_converter():
    from unmanned_aerial_vehicles_amd._lib import host_ptr
    a = np.arange(12.0).reshape(4, 3)
    p = host_ptr(a)
    assert isinstance(p, ctypes.POINTER(ctypes.c_double))
    assert ctypes.cast(p, ctypes.c_void_p).value == a.ctypes.data and p[5] == 5.0
    assert host_ptr(None) is None
    # a read-only array and an empty one export no writable buffer: the same pointer by the slower route
    ro = np.arange(3.0)
    ro.setflags(write=False)
    assert ctypes.cast(host_ptr(ro), ctypes.c_void_p).value == ro.ctypes.data and host_ptr(ro)[2] == 2.0
    assert isinstance(host_ptr(np.empty((0, 3))), ctypes.POINTER(ctypes.c_double))
    # the pointer keeps the array alive
    p2 = host_ptr(np.full(4, 7.0))
    assert p2[3] == 7.0
    with pytest.raises(TypeError):
        host_ptr(a.astype(np.float32))
    with pytest.raises(TypeError):
        host_ptr(np.zeros((4, 3))[:, ::2])
    with pytest.raises(TypeError):
        host_ptr([1.0, 2.0])
    with pytest.raises(TypeError):
        host_ptr(np.asfortranarray(a))


def test_device_pointer_converter():
    from unmanned_aerial_vehicles_amd._lib import dev_ptr

    class _T:
        def data_ptr(self):
            return 0x7F00DEAD0000

    p = dev_ptr(_T())
    assert isinstance(p, ctypes.c_void_p) and p.value == 0x7F00DEAD0000
    assert dev_ptr(None) is None


def test_aliases_kept_for_importers():
    from unmanned_aerial_vehicles_amd import _lib, device, sparse
    assert device._p is _lib.dev_ptr and sparse._ptr is _lib.host_ptr
    assert not hasattr(_lib, "dptr")


def test_check_queries():
    from unmanned_aerial_vehicles_amd.device import check_queries
    X = check_queries([1.0, 2.0, 3.0])
    assert X.shape == (1, 3) and X.dtype == np.float64 and X.flags.c_contiguous
    assert check_queries(np.zeros((4, 6))[:, ::2], 3).flags.c_contiguous
    with pytest.raises(ValueError, match=r"^Input X contains NaN or infinity\.$"):
        check_queries([[1.0, np.inf]])
    with pytest.raises(ValueError, match=r"^Input X contains NaN or infinity\.$"):
        check_queries([[np.nan, 1.0]], 5)          # (the finiteness check comes first, as in every caller)
    with pytest.raises(ValueError, match=r"^queries must be \(M, 4\)$"):
        check_queries(np.zeros((2, 3)), 4)
    with pytest.raises(ValueError, match=r"^queries must be \(M, 3\)$"):
        check_queries(np.zeros((2, 2, 3)), 3)
    assert check_queries(np.zeros((2, 3))).shape == (2, 3)     # no width given: none checked


def _outside_class_backend(src):
    """`src` without the body of `class Backend` (from its `class` line to the next line that starts in column 0)."""
    m = re.search(r"^class Backend\b.*?(?=^\S)", src, flags=re.M | re.S)
    return src if m is None else src[:m.start()] + src[m.end():]


def test_the_package_enters_the_library_only_through_backend():
    pkg = os.path.join(ROOT, "unmanned_aerial_vehicles_amd")
    seen_backend = False
    for fn in sorted(os.listdir(pkg)):
        if not fn.endswith(".py"):
            continue
        src = open(os.path.join(pkg, fn)).read()
        rest = _outside_class_backend(src)
        seen_backend |= rest != src
        for pat in (r"\.lib\.gpk_", r"bind_stream\("):
            hits = [ln for ln in rest.splitlines() if re.search(pat, ln)]
            assert not hits, f"{fn}: {pat} outside class Backend: {hits[:3]}"
        if fn != "_lib.py":
            hits = [ln for ln in src.splitlines() if re.search(r"data_as\((_lib\.)?_dp\)", ln)]
            assert not hits, f"{fn}: a double-pointer conversion outside _lib.py: {hits[:3]}"
    assert seen_backend, "class Backend not found: the exclusion above matched nothing"
