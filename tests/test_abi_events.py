"""The completion-handle entries of the C-ABI (include/pa_hip.h: the async
exchange and pa_event): declared, exported, and failing loudly on bad
arguments (no compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

ENTRIES = ["pa_exchange_all_async", "pa_mat_exchange_all_async", "pa_event_record", "pa_event_query",
           "pa_event_wait", "pa_ctx_wait_event", "pa_event_destroy"]


def test_header_declares_the_event_entries():
    src = open(HEADER).read()
    names = set(re.findall(r"^\s*int\s+(pa_\w+)\s*\(", src, re.M))
    for e in ENTRIES:
        assert e in names, e
    assert re.search(r"typedef\s+struct\s+pa_event\s+pa_event\s*;", src)


def test_library_exports_the_event_entries(pamd):
    L = pamd._lib.lib()
    for e in ENTRIES:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    vp = ctypes.c_void_p
    d = ctypes.c_int(-7)
    assert L.pa_event_query(None, ctypes.byref(d)) != 0 and len(L.pa_last_error()) > 0
    assert d.value == -7  # untouched
    one = (vp * 1)()
    done = (vp * 1)()
    # n = 0
    assert L.pa_exchange_all_async(0, one, one, None, 0, 0, 0, None, done) != 0
    assert len(L.pa_last_error()) > 0 and not done[0]
    # a null done
    assert L.pa_exchange_all_async(1, one, one, None, 0, 0, 0, None, None) != 0
    assert b"done" in L.pa_last_error()
    assert L.pa_mat_exchange_all_async(1, one, one, 0, 0, 0, None, None) != 0
    assert b"done" in L.pa_last_error()
    # null handles inside the arrays
    assert L.pa_exchange_all_async(1, one, one, None, 0, 0, 0, None, done) != 0
    assert len(L.pa_last_error()) > 0 and not done[0]
    assert L.pa_mat_exchange_all_async(1, one, one, 0, 0, 0, None, done) != 0
    assert len(L.pa_last_error()) > 0 and not done[0]
    h = vp()
    assert L.pa_event_record(None, ctypes.byref(h)) != 0 and not h.value
    assert L.pa_event_wait(None) != 0 and len(L.pa_last_error()) > 0
    assert L.pa_ctx_wait_event(None, None) != 0 and len(L.pa_last_error()) > 0
    assert L.pa_event_destroy(None) == 0  # as the other *_destroy
