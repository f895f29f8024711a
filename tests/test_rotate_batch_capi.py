"""The C-ABI surface of the batched same-key rotations, as far as it goes without a device: the three
entry points are declared in include/phantom_amd.h, exported by the library and bound by the ctypes
module with the declared arity, each refuses a null context before touching anything, and the
binding has its helpers.  (What they compute is tests/test_gpu_rotate_many.py's.)"""
import ctypes
import re

import pytest

import phantom_amd as PA

NAMES = ["phantom_keyswitch_rotate_many", "phantom_rotate_fused_batch", "phantom_rotate_fused_batch_chunk"]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    assert name in PA.declared_symbols()
    fn = getattr(PA.load(), name)  # AttributeError if the library does not export it
    txt = re.sub(r"/\*.*?\*/", "", open(PA.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params.split(",")), params


def test_null_context_is_refused_with_a_message():
    lib = PA.load()
    chunk = ctypes.c_size_t(77)
    calls = [
        lambda: lib.phantom_keyswitch_rotate_many(None, 1, 1, None, None, None, 0, 3, None, None),
        lambda: lib.phantom_rotate_fused_batch(None, 1, 0, None, None, 0, 3, None, None),
        lambda: lib.phantom_rotate_fused_batch_chunk(None, 1, ctypes.byref(chunk)),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert lib.phantom_last_error(), i
    assert chunk.value == 77


def test_binding_helpers():
    for helper in ("rotate_fused_batch", "rotate_fused_batch_chunk", "keyswitch_rotate_many"):
        assert callable(getattr(PA, helper))
