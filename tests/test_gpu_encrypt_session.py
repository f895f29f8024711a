"""phantom_boot_encrypt_device / phantom_boot_decrypt_device: a bootstrap session's batched
device-to-device encryption and decryption beside its host-path entries (phantom_boot_encrypt /
phantom_boot_decrypt), on a session at N = 2^12 with the default chain (Q = {60, 29 x 59}, P = 10 x 60)
and on one sparse session with N/8 slots.  Inputs uniform in [1, 5], chain index 26, three ciphertexts.

A session key encrypts from OS entropy, so nothing here is bit-compared between paths: the round
trips meet the precision bar of tests/test_gpu_bootstrap.py (bit_precision > 30), the device
decryption of one host-encrypted ciphertext errs at most 4 x as much as the host decryption of the
same bytes, and the serialized header is the host entry's."""
import ctypes

import numpy as np
import pytest

import phantom_amd as PA
from test_serialize import Hdr

pytestmark = pytest.mark.gpu

LOG_N, CHAIN, COUNT = 12, 26, 3


def torch():
    import torch as t
    return t


def header(blob):
    h, words = Hdr(), ctypes.c_size_t(0)
    PA.check(PA.load().phantom_ciphertext_deserialize(blob, len(blob), ctypes.byref(h), None, 0, ctypes.byref(words)))
    return h, words.value


class Case:
    def __init__(self, num_slots):
        t = torch()
        self.sess = PA.BootSession(bytes(range(32)), log_n=LOG_N, num_slots=num_slots)
        self.slots = self.sess.slots
        rng = np.random.default_rng(0xE0 + num_slots)
        self.vals = rng.uniform(1.0, 5.0, size=(COUNT, self.slots))
        self.sin = self.sess.input_bytes(CHAIN)
        self.host_ct = t.zeros((COUNT, self.sin), dtype=t.uint8, device="cuda")
        assert self.sess.encrypt(self.vals, CHAIN, self.host_ct.data_ptr(), self.sin) == self.sin
        self.dev_ct = t.zeros((COUNT, self.sin), dtype=t.uint8, device="cuda")
        dv = t.from_numpy(self.vals.astype(np.complex128)).cuda()
        t.cuda.synchronize()
        assert self.sess.encrypt_device(dv.data_ptr(), COUNT, CHAIN, self.dev_ct.data_ptr(), self.sin) == self.sin
        t.cuda.synchronize()

    def decrypt(self, cts):
        return np.stack([self.sess.decrypt(cts[i].data_ptr(), self.sin) for i in range(COUNT)])

    def decrypt_device(self, cts):
        t = torch()
        out = t.zeros((COUNT, self.slots), dtype=t.complex128, device="cuda")
        t.cuda.synchronize()
        self.sess.decrypt_device(cts.data_ptr(), self.sin, COUNT, out.data_ptr())
        t.cuda.synchronize()
        return out.cpu().numpy()


_cases = {}


def case(num_slots):
    if num_slots not in _cases:
        _cases[num_slots] = Case(num_slots)
    return _cases[num_slots]


@pytest.mark.parametrize("num_slots", [0, (1 << LOG_N) // 8])
def test_all_four_encrypt_decrypt_paths_reach_the_precision_bar(num_slots):
    c = case(num_slots)
    for enc_name, cts in (("encrypt", c.host_ct), ("encrypt_device", c.dev_ct)):
        host = c.decrypt(cts)
        dev = c.decrypt_device(cts)
        assert np.max(np.abs(dev.imag)) < 1e-6  # real inputs decode to real slots
        for i in range(COUNT):
            bits = (PA.bit_precision(c.vals[i], host[i]), PA.bit_precision(c.vals[i], dev[i].real))
            print(f"slots {c.slots} {enc_name} ciphertext {i}: decrypt {bits[0]:.2f} bits, decrypt_device {bits[1]:.2f} bits")
            assert min(bits) > 30, (enc_name, i, bits)


@pytest.mark.parametrize("num_slots", [0, (1 << LOG_N) // 8])
def test_decrypt_device_error_against_decrypt_of_the_same_bytes(num_slots):
    c = case(num_slots)
    e_host = float(np.max(np.abs(c.decrypt(c.host_ct) - c.vals)))
    e_dev = float(np.max(np.abs(c.decrypt_device(c.host_ct).real - c.vals)))
    print(f"slots {c.slots}: decrypt error {e_host:.3e}, decrypt_device error {e_dev:.3e}")
    assert e_host > 0 and e_dev <= 4 * e_host


@pytest.mark.parametrize("num_slots", [0, (1 << LOG_N) // 8])
def test_encrypt_device_writes_the_host_entrys_header(num_slots):
    c = case(num_slots)
    for i in range(COUNT):
        want, w_words = header(bytes(c.host_ct[i].cpu().numpy()))
        got, g_words = header(bytes(c.dev_ct[i].cpu().numpy()))
        assert g_words == w_words == (c.sin - 58) // 8
        for name, _ in Hdr._fields_:
            assert getattr(got, name) == getattr(want, name), (i, name)
        assert got.chain_index == CHAIN and got.size == 2 and got.is_ntt_form and not got.is_asymmetric


def test_bootstrap_of_device_encrypted_inputs():
    c = case(0)
    t = torch()
    sout = c.sess.output_bytes()
    out = t.zeros((2, sout), dtype=t.uint8, device="cuda")
    c.sess.run(c.dev_ct.data_ptr(), c.sin, 2, out.data_ptr(), sout, 1)
    t.cuda.synchronize()
    vals = t.zeros((2, c.slots), dtype=t.complex128, device="cuda")
    t.cuda.synchronize()
    c.sess.decrypt_device(out.data_ptr(), sout, 2, vals.data_ptr())
    t.cuda.synchronize()
    bits = [PA.bit_precision(c.vals[i], vals[i].cpu().numpy().real) for i in range(2)]
    print("bootstrap of device-encrypted inputs, decrypt_device:", bits)
    assert min(bits) > 9.85, bits


def test_session_bad_arguments():
    c = case(0)
    lib, h = PA.load(), c.sess.handle
    b = ctypes.c_size_t(0)
    t = torch()
    vals = t.zeros((1, c.slots), dtype=t.complex128, device="cuda")
    out = t.zeros(c.sin, dtype=t.uint8, device="cuda")
    assert lib.phantom_boot_encrypt_device(h, None, 1, CHAIN, out.data_ptr(), c.sin, ctypes.byref(b)) == 1
    assert lib.phantom_boot_encrypt_device(h, vals.data_ptr(), 1, CHAIN, None, c.sin, ctypes.byref(b)) == 1
    assert lib.phantom_boot_encrypt_device(h, vals.data_ptr(), 1, 0, out.data_ptr(), c.sin, ctypes.byref(b)) == 1
    assert lib.phantom_boot_encrypt_device(h, vals.data_ptr(), 1, CHAIN, out.data_ptr(), c.sin - 1, ctypes.byref(b)) == 1
    assert b.value == c.sin  # the needed size is reported all the same
    assert lib.phantom_boot_decrypt_device(h, None, c.sin, 1, vals.data_ptr()) == 1
    assert lib.phantom_boot_decrypt_device(h, c.dev_ct.data_ptr(), c.sin, 0, vals.data_ptr()) == 1
    assert lib.phantom_boot_decrypt_device(h, c.dev_ct.data_ptr(), c.sin - 8, 1, vals.data_ptr()) == 1  # truncated
    assert lib.phantom_boot_decrypt_device(h, out.data_ptr(), c.sin, 1, vals.data_ptr()) == 1  # zero header
    t.cuda.synchronize()
    assert not out.any() and not vals.view(t.float64).any()
