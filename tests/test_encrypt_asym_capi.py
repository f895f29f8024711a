"""The C-ABI surface of the batched public-key encryption, as far as it goes without a device: the three
entry points are declared in include/phantom_amd.h, exported by the library and bound by the ctypes
module with the declared arity, and each refuses a null context with PHANTOM_ERR_INVALID_ARGUMENT and a
message before touching anything.  (What they compute is tests/test_gpu_encrypt_asym_batch.py's.)"""
import ctypes
import re

import numpy as np
import pytest

import phantom_amd as PA

NAMES = ["phantom_encrypt_asymmetric_batch", "phantom_encrypt_asymmetric_batch_chunk", "phantom_sample_small_batch"]


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(name):
    assert name in PA.declared_symbols()
    fn = getattr(PA.load(), name)  # AttributeError if the library does not export it
    txt = re.sub(r"/\*.*?\*/", "", open(PA.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params.split(",")), params


def test_null_context_is_refused_with_a_message():
    lib = PA.load()
    key = np.arange(8, dtype=np.uint32)
    nonces = np.arange(3, dtype=np.uint64)
    chunk = ctypes.c_size_t(77)
    calls = [
        lambda: lib.phantom_encrypt_asymmetric_batch(None, 1, None, None, 0, 0, 1.0, 1, key.ctypes.data,
                                                     nonces.ctypes.data, None, 0, None, None),
        lambda: lib.phantom_sample_small_batch(None, 1, key.ctypes.data, nonces.ctypes.data, 3, None, None),
        lambda: lib.phantom_encrypt_asymmetric_batch_chunk(None, 1, ctypes.byref(chunk)),
    ]
    for i, call in enumerate(calls):
        assert call() == 1, i
        assert lib.phantom_last_error(), i
    assert chunk.value == 77


def test_public_encryptor_wrapper_mirrors_encryptor():
    for method in ("chunk", "sample_small", "encrypt"):
        assert callable(getattr(PA.PublicEncryptor, method))
    assert (PA.PublicEncryptor.CBD, PA.PublicEncryptor.TERNARY) == (1, 2)  # PHANTOM_SAMPLE_CBD / _TERNARY
    with pytest.raises(AssertionError):
        PA.PublicEncryptor(None, 0, np.zeros(7, dtype=np.uint32))
