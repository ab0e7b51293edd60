"""CPU checks of the instance-state surface (snapshot, restore, reset): the C ABI declares and exports it, the Python mirror binds it, and
the mirror refuses bad arguments before anything reaches the library -- no GPU needed."""
import ctypes as C
import os
import re

import pytest

from oalsfxpp_amd import api, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("oalsfx_batch_snapshot_bytes", "oalsfx_batch_snapshot", "oalsfx_batch_restore", "oalsfx_batch_reset")


def test_header_declares_and_the_mirror_binds_the_state_calls():
    header = open(os.path.join(ROOT, "include", "oalsfx_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in lib.SIGNATURES, name
    assert lib.SIGNATURES["oalsfx_batch_snapshot_bytes"][0] is C.c_ulonglong


def test_the_library_exports_the_state_calls():
    so = C.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(so, name), name


def test_the_array_header_declares_reset():
    header = open(os.path.join(ROOT, "include", "oalsfxpp_array.h")).read()
    assert re.search(r"bool reset\(int index\);", header)


def _unopened(n=8):
    """A Batch whose handle was never created: a check that let a call through would fail on the missing library, not with BatchError."""
    b = api.Batch.__new__(api.Batch)
    b.n = n
    b._h = None
    b._lib = None
    return b


@pytest.mark.parametrize("instances", [[8], [-1], [0, 9], "abc", [0.5], [None]])
def test_instance_lists_out_of_range_are_refused(instances):
    b = _unopened()
    for call in (lambda: b.snapshot_bytes(instances), lambda: b.reset(instances), lambda: b.snapshot(instances, 0x1000, 4096),
                 lambda: b.restore(instances, 0x1000, 4096)):
        with pytest.raises(api.BatchError):
            call()


def test_restore_refuses_duplicate_targets():
    with pytest.raises(api.BatchError, match="twice"):
        _unopened().restore([1, 2, 1], 0x1000, 4096)


@pytest.mark.parametrize("ptr, nbytes, what", [(0, 4096, "No snapshot buffer"), (0x1008, 4096, "aligned"), (0x1004, 4096, "aligned"),
                                               (0x1000, -1, "negative")])
def test_buffers_are_checked(ptr, nbytes, what):
    b = _unopened()
    with pytest.raises(api.BatchError, match=what):
        b.snapshot([0], ptr, nbytes)
    with pytest.raises(api.BatchError, match=what):
        b.restore([0], ptr, nbytes)
