"""ctypes binding of libphantom_amd.so (include/phantom_amd.h) for tests and bench.py.

The product is the C-ABI library; this module only loads it and declares signatures.
It raises if the library is missing — there is no Python or CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PHANTOM_AMD_LIB: load another build of the same library (tools/build_variants.sh experiments)
LIB_PATH = os.environ.get("PHANTOM_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libphantom_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "phantom_amd.h")

u64p = ctypes.POINTER(ctypes.c_uint64)
vp = ctypes.c_void_p
sz = ctypes.c_size_t

_SIGS = {
    "phantom_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "phantom_last_error": (ctypes.c_char_p, []),
    "phantom_version": (ctypes.c_char_p, []),
    "phantom_coeff_modulus_create": (ctypes.c_int, [sz, ctypes.POINTER(ctypes.c_int), sz, u64p]),
    "phantom_ntt_tables_create": (ctypes.c_int, [sz, u64p, sz, ctypes.POINTER(vp)]),
    "phantom_ntt_tables_destroy": (ctypes.c_int, [vp]),
    "phantom_ntt_tables_host": (ctypes.c_int, [vp, sz, u64p, u64p, u64p, u64p, u64p]),
    "phantom_nwt_forward_inplace": (ctypes.c_int, [vp, vp, sz, sz, vp]),
    "phantom_nwt_backward_inplace": (ctypes.c_int, [vp, vp, sz, sz, vp]),
    "phantom_nwt_backward": (ctypes.c_int, [vp, vp, vp, sz, sz, vp]),
    "phantom_nwt_backward_scale": (ctypes.c_int, [vp, vp, vp, sz, sz, vp, vp, vp]),
    "phantom_nwt_forward_include_special_mod_exclude_range": (ctypes.c_int, [vp, vp, sz, sz, sz, sz, sz, sz, vp]),
    "phantom_nwt_backward_inplace_include_special_mod": (ctypes.c_int, [vp, vp, sz, sz, sz, sz, vp]),
    "phantom_nwt_backward_inplace_scale": (ctypes.c_int, [vp, vp, sz, sz, vp, vp, vp]),
    "phantom_nwt_forward_include_special_mod": (ctypes.c_int, [vp, vp, sz, sz, sz, sz, vp]),
    "phantom_nwt_forward_fuse_moddown": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, sz, sz, vp]),
    "phantom_fnwt_1d": (ctypes.c_int, [vp, vp, sz, sz, vp]),
    "phantom_inwt_1d": (ctypes.c_int, [vp, vp, sz, sz, vp, vp, vp]),
    "phantom_context_create": (ctypes.c_int, [sz, u64p, sz, sz, ctypes.POINTER(vp)]),
    "phantom_context_destroy": (ctypes.c_int, [vp]),
    "phantom_context_coeff_modulus_size": (sz, [vp, sz]),
    "phantom_context_set_unbiased_moddown": (ctypes.c_int, [vp, ctypes.c_int]),
    "phantom_multiply": (ctypes.c_int, [vp, sz, vp, vp, vp, vp]),
    "phantom_square": (ctypes.c_int, [vp, sz, vp, vp, vp]),
    "phantom_relinearize": (ctypes.c_int, [vp, sz, vp, ctypes.POINTER(vp), sz, vp]),
    "phantom_relinearize_rescale": (ctypes.c_int, [vp, sz, vp, vp, ctypes.POINTER(vp), sz, vp]),
    "phantom_relinearize_rescale_batch": (ctypes.c_int, [vp, sz, vp, sz, sz, vp, sz, ctypes.POINTER(vp), sz, vp]),
    "phantom_keyswitch": (ctypes.c_int, [vp, sz, vp, vp, ctypes.POINTER(vp), sz, vp]),
    "phantom_modup": (ctypes.c_int, [vp, sz, vp, vp, vp]),
    "phantom_keyswitch_inner_prod": (ctypes.c_int, [vp, sz, vp, ctypes.POINTER(vp), sz, vp, vp]),
    "phantom_moddown_from_ntt": (ctypes.c_int, [vp, sz, vp, vp, vp]),
    "phantom_fast_bconv": (ctypes.c_int, [u64p, sz, u64p, sz, vp, vp, sz, ctypes.c_int, vp]),
    "phantom_bconv_create": (ctypes.c_int, [u64p, sz, u64p, sz, vp, ctypes.POINTER(vp)]),
    "phantom_bconv_run": (ctypes.c_int, [vp, vp, vp, sz, ctypes.c_int, vp]),
    "phantom_bconv_destroy": (ctypes.c_int, [vp]),
    "phantom_moddown_modup": (ctypes.c_int, [vp, sz, vp, vp, vp]),
    "phantom_moddown_modup_batch": (ctypes.c_int, [vp, sz, vp, sz, sz, vp, vp]),
    "phantom_ciphertext_serialize": (ctypes.c_int, [vp, vp, vp, sz, vp]),
    "phantom_ciphertext_deserialize": (ctypes.c_int, [vp, sz, vp, vp, sz, vp]),
    "phantom_moddown_rescale": (ctypes.c_int, [vp, sz, vp, vp, sz, vp]),
    "phantom_rescale_to_next": (ctypes.c_int, [vp, sz, vp, vp, sz, vp]),
    "phantom_apply_galois_ntt": (ctypes.c_int, [vp, ctypes.c_uint32, vp, vp, sz, vp]),
    "phantom_poly_op": (ctypes.c_int, [vp, ctypes.c_int, vp, vp, vp, sz, sz, vp]),
    "phantom_switch_modulus_raise": (ctypes.c_int, [vp, vp, vp, sz, vp]),
    "phantom_chacha20_block": (ctypes.c_int, [vp, ctypes.c_uint64, ctypes.c_uint64, vp]),
    "phantom_sample_poly": (ctypes.c_int, [vp, ctypes.c_int, vp, ctypes.c_uint64, vp, sz, vp]),
    "phantom_boot_session_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint32,
                                                   ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.POINTER(vp)]),
    "phantom_boot_session_destroy": (ctypes.c_int, [vp]),
    "phantom_traffic_read": (ctypes.c_int, [vp]),
    "phantom_traffic_reset": (ctypes.c_int, []),
    "phantom_pool_stats": (ctypes.c_int, [vp]),
    "phantom_pool_reset_peak": (ctypes.c_int, []),
    "phantom_lt_bsgs": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), vp]),
    "phantom_keyswitch_ext": (ctypes.c_int, [vp, sz, vp, vp, vp]),
    "phantom_fast_rotation_ext": (ctypes.c_int, [vp, sz, vp, vp, ctypes.POINTER(vp), sz, ctypes.c_uint32, ctypes.c_int,
                                                 vp, vp]),
    "phantom_fast_rotation_ext_batch": (ctypes.c_int, [vp, sz, vp, vp, ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                                       ctypes.POINTER(ctypes.c_uint32), sz, ctypes.POINTER(vp), vp]),
    "phantom_rotate_ext_accumulate": (ctypes.c_int, [vp, sz, vp, ctypes.POINTER(vp), sz, ctypes.c_uint32, vp,
                                                     ctypes.c_int, vp]),
    "phantom_lt_bsgs_group": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), sz, sz, ctypes.POINTER(vp), sz,
                                             ctypes.POINTER(vp), ctypes.POINTER(vp), sz, vp]),
    "phantom_fast_rotation_ext_batch_group": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                             ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                                             ctypes.POINTER(ctypes.c_uint32), sz, ctypes.POINTER(vp),
                                                             vp]),
    "phantom_rotate_ext_accumulate_group": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), sz,
                                                           ctypes.c_uint32, ctypes.POINTER(vp), ctypes.c_int, vp]),
    "phantom_tensor_lin": (ctypes.c_int, [vp, sz, vp, vp, vp, vp, vp, sz, vp, vp]),
    "phantom_tensor_lin_batch": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                vp, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), ctypes.POINTER(vp), vp]),
    "phantom_lin_comb": (ctypes.c_int, [vp, sz, vp, sz, vp, vp, sz, sz, vp, vp]),
    "phantom_mul_scalar": (ctypes.c_int, [vp, sz, vp, sz, vp, vp, vp, sz, vp]),
    "phantom_leaf_combine": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), vp, sz, vp, vp, ctypes.POINTER(vp), sz, vp]),
    "phantom_eval_mod_coefficients": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, vp]),
    "phantom_boot_encrypt": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_boot_output_bytes": (ctypes.c_int, [vp, ctypes.POINTER(sz)]),
    "phantom_galois_key_serialize": (ctypes.c_int, [sz, sz, sz, sz, vp, vp, sz, vp]),
    "phantom_salsa20_block": (ctypes.c_int, [vp, ctypes.c_uint64, vp]),
    "phantom_sample_uniform_seeded": (ctypes.c_int, [vp, vp, vp, sz, vp]),
    "phantom_boot_layout": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint32,
                                           ctypes.c_uint32, sz, ctypes.POINTER(sz), ctypes.POINTER(sz),
                                           ctypes.POINTER(sz)]),
    "phantom_boot_run": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, ctypes.c_int]),
    "phantom_boot_run_grouped": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, ctypes.c_int, ctypes.c_int]),
    "phantom_boot_decrypt": (ctypes.c_int, [vp, vp, sz, vp]),
    "phantom_ckks_embed": (ctypes.c_int, [vp, ctypes.c_int, vp, vp, sz, sz, vp]),
    "phantom_ckks_round_rns": (ctypes.c_int, [vp, sz, ctypes.c_int, vp, ctypes.c_double, sz, ctypes.c_int, vp, vp, vp]),
    "phantom_ckks_compose": (ctypes.c_int, [vp, sz, vp, sz, vp, vp]),
    "phantom_ckks_encode": (ctypes.c_int, [vp, sz, ctypes.c_int, vp, sz, sz, ctypes.c_double, sz, vp, vp, vp]),
    "phantom_ckks_decode": (ctypes.c_int, [vp, sz, vp, ctypes.c_double, sz, vp, vp]),
    "phantom_ltprep_stage_offsets": (ctypes.c_int, [sz, vp, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_ltprep_stage_products": (ctypes.c_int, [vp, sz, ctypes.c_int, vp, sz, vp, vp, sz, vp]),
    "phantom_ltprep_stage_products_host": (ctypes.c_int, [sz, ctypes.c_int, vp, sz, vp, sz]),
    "phantom_ltprep_presence": (ctypes.c_int, [vp, sz, vp, sz, ctypes.c_double, ctypes.c_double, ctypes.c_int, vp, vp]),
    "phantom_ltprep_lifted_offsets": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_ltprep_shape": (ctypes.c_int, [sz, vp, sz, ctypes.c_int, ctypes.c_uint32, vp]),
    "phantom_ltprep_finish": (ctypes.c_int, [vp, sz, sz, vp, sz, vp, sz, vp, ctypes.c_double, ctypes.c_double,
                                             ctypes.c_int, ctypes.c_int, vp, vp, vp]),
    "phantom_ltprep_finish_host": (ctypes.c_int, [vp, sz, sz, vp, sz, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_uint32, vp, vp, vp, sz,
                                                  ctypes.POINTER(sz), vp]),
    "phantom_ltprep_dense_diagonals": (ctypes.c_int, [vp, sz, ctypes.c_double, vp, vp, vp]),
    "phantom_boot_session_create_opts": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_uint32,
                                                        ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint32,
                                                        ctypes.POINTER(vp)]),
    "phantom_sample_cbd_small_batch": (ctypes.c_int, [vp, vp, vp, sz, vp, vp]),
    "phantom_encrypt_symmetric_batch": (ctypes.c_int, [vp, sz, vp, vp, sz, sz, ctypes.c_double, sz, vp, vp, vp, vp, sz,
                                                       vp, vp]),
    "phantom_decrypt_batch": (ctypes.c_int, [vp, vp, vp, sz, sz, sz, sz, sz, vp, vp]),
    "phantom_decrypt_decode_batch": (ctypes.c_int, [vp, vp, vp, sz, sz, sz, sz, sz, ctypes.c_double, vp, vp]),
    "phantom_encrypt_batch_chunk": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    "phantom_sample_small_batch": (ctypes.c_int, [vp, ctypes.c_int, vp, vp, sz, vp, vp]),
    "phantom_encrypt_asymmetric_batch": (ctypes.c_int, [vp, sz, vp, vp, sz, sz, ctypes.c_double, sz, vp, vp, vp, sz, vp,
                                                        vp]),
    "phantom_encrypt_asymmetric_batch_chunk": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    "phantom_boot_encrypt_device": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_boot_decrypt_device": (ctypes.c_int, [vp, vp, sz, sz, vp]),
    "phantom_ct_mix": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, vp, vp, ctypes.POINTER(vp), sz, vp]),
    "phantom_rotate_sum_ext": (ctypes.c_int, [vp, sz, vp, vp, ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                              ctypes.POINTER(ctypes.c_uint32), sz, ctypes.c_int, vp, vp]),
    "phantom_avgpool_rotations": (ctypes.c_int, [sz, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_avgpool_fc": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, sz, sz, sz, vp, vp,
                                          ctypes.POINTER(ctypes.POINTER(vp)), ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(vp), vp]),
    "phantom_pack_rotations": (ctypes.c_int, [sz, sz, sz, sz, vp, vp, vp, sz, ctypes.POINTER(sz)]),
    "phantom_ct_pack": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, ctypes.c_uint32, vp, vp]),
    "phantom_ct_split": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), sz, ctypes.c_uint32,
                                        ctypes.POINTER(vp), ctypes.POINTER(vp), vp]),
    "phantom_keyswitch_rotate_many": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                                     ctypes.POINTER(vp), sz, ctypes.c_uint32, ctypes.POINTER(vp), vp]),
    "phantom_rotate_fused_batch": (ctypes.c_int, [vp, sz, sz, ctypes.POINTER(vp), ctypes.POINTER(vp), sz,
                                                  ctypes.c_uint32, ctypes.POINTER(vp), vp]),
    "phantom_rotate_fused_batch_chunk": (ctypes.c_int, [vp, sz, ctypes.POINTER(sz)]),
    "phantom_conv_rotations": (ctypes.c_int, [sz, sz, sz, vp, sz, ctypes.POINTER(sz)]),
    "phantom_conv_weight_slots": (ctypes.c_int, [sz, sz, sz, sz, sz, vp, sz, sz, vp, vp]),
    "phantom_conv_weight_slots_host": (ctypes.c_int, [sz, sz, sz, sz, sz, vp, sz, sz, vp]),
    "phantom_ext_mac": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, vp, sz, ctypes.POINTER(vp), ctypes.c_int, vp]),
    "phantom_conv2d": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, sz, sz, sz, sz, vp, ctypes.c_double,
                                      ctypes.POINTER(ctypes.POINTER(vp)), sz, ctypes.POINTER(ctypes.c_uint32), sz,
                                      ctypes.POINTER(vp), vp, vp]),
    "phantom_ckks_encode_sub": (ctypes.c_int, [vp, sz, ctypes.c_int, vp, sz, sz, ctypes.c_double, sz, vp, vp, vp]),
    "phantom_sub_ntt": (ctypes.c_int, [vp, sz, ctypes.c_int, sz, ctypes.c_int, vp, sz, vp]),
    "phantom_ext_mac_sub": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, vp, sz, sz, ctypes.POINTER(vp), ctypes.c_int,
                                           vp]),
    "phantom_conv2d_prepare": (ctypes.c_int, [vp, sz, sz, sz, sz, sz, sz, vp, ctypes.c_double, vp, vp,
                                              ctypes.POINTER(vp)]),
    "phantom_conv_plan_bytes": (ctypes.c_int, [vp, ctypes.POINTER(sz)]),
    "phantom_conv_plan_destroy": (ctypes.c_int, [vp]),
    "phantom_conv2d_apply": (ctypes.c_int, [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(vp), vp]),
    "phantom_ext_mac_sub_seeded": (ctypes.c_int, [vp, sz, ctypes.POINTER(vp), sz, vp, sz, sz, ctypes.POINTER(vp),
                                                  ctypes.POINTER(vp), vp, vp, vp]),
    "phantom_conv2d_prepare_scaled": (ctypes.c_int, [vp, sz, sz, sz, sz, sz, sz, vp, vp, ctypes.c_double, vp, vp,
                                                     ctypes.POINTER(vp)]),
    "phantom_conv2d_apply_seeded": (ctypes.c_int, [vp, vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.POINTER(vp)), sz,
                                                   ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(vp),
                                                   ctypes.POINTER(vp), vp, vp, vp]),
    "phantom_conv_plan_read": (ctypes.c_int, [vp, vp, sz]),
    "phantom_scaled_constant_residues": (ctypes.c_int, [ctypes.c_double, ctypes.c_double, vp, sz, vp]),
}

_lib = None


class PhantomError(RuntimeError):
    pass


def load():
    """Load libphantom_amd.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch bundles its own libamdhip64 (soname
        # libamdhip64.so.7).  Loading torch first makes this library bind to that same
        # runtime instead of pulling a second copy from /opt/rocm.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise PhantomError(f"{LIB_PATH} missing: run __graft_entry__.build() (no fallback path exists)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    return _lib


def check(status):
    if status != 0:
        lib = load()
        raise PhantomError(f"{lib.phantom_status_string(status).decode()}: {lib.phantom_last_error().decode()}")


def declared_symbols(header=HEADER_PATH):
    """Names of every function declared in include/phantom_amd.h."""
    import re
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(phantom_[a-z0-9_]+)\s*\(", txt)))


def u64_array(values):
    arr = (ctypes.c_uint64 * len(values))(*values)
    return arr


def coeff_modulus_create(n, bit_sizes):
    lib = load()
    bs = (ctypes.c_int * len(bit_sizes))(*bit_sizes)
    out = (ctypes.c_uint64 * len(bit_sizes))()
    check(lib.phantom_coeff_modulus_create(n, bs, len(bit_sizes), out))
    return list(out)


class Context:
    """Owning handle of a phantom_context (CKKS PhantomContext over a key-level chain)."""

    def __init__(self, n, moduli, special_modulus_size):
        lib = load()
        self.n = n
        self.moduli = list(moduli)
        self.size_P = special_modulus_size
        self.size_Q = len(self.moduli) - special_modulus_size
        h = vp()
        check(lib.phantom_context_create(n, u64_array(self.moduli), len(self.moduli), special_modulus_size,
                                         ctypes.byref(h)))
        self.handle = h

    def ql(self, chain_index):
        return self.moduli[:self.size_Q - (chain_index - 1)]

    def set_unbiased_moddown(self, on):
        """Opt-in mean-unbiased moddowns (phantom_context_set_unbiased_moddown); off by default."""
        check(load().phantom_context_set_unbiased_moddown(self.handle, 1 if on else 0))

    def close(self):
        if self.handle:
            load().phantom_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Encoder:
    """CKKS encode / decode on the device (phantom_ckks_*): every argument that names data is a
    device pointer (e.g. a torch tensor's data_ptr()): slot values are complex128 (interleaved
    re, im doubles), coefficients float64, plaintexts int64 / uint64 words [count][limbs][n].
    Calls enqueue on `stream` and return; nothing is synchronised."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.n = ctx.n
        self.slots = ctx.n // 2

    def limbs(self, chain_index, ext=False):
        """words of one plaintext at chain_index are limbs * n"""
        return load().phantom_context_coeff_modulus_size(self.ctx.handle, chain_index) + (self.ctx.size_P if ext else 0)

    def embed(self, forward, src, dst, stream, sparse_slots=0, count=1):
        check(load().phantom_ckks_embed(self.ctx.handle, 1 if forward else 0, src, dst, sparse_slots, count, stream))

    def round_rns(self, chain_index, coeffs, scale, out, stream, ext=False, count=1, ntt_form=True, overflow=None):
        check(load().phantom_ckks_round_rns(self.ctx.handle, chain_index, 1 if ext else 0, coeffs, scale, count,
                                            1 if ntt_form else 0, out, overflow, stream))

    def compose(self, chain_index, plain, coeffs, stream, count=1):
        check(load().phantom_ckks_compose(self.ctx.handle, chain_index, plain, count, coeffs, stream))

    def encode(self, chain_index, values, num_values, scale, out, stream, ext=False, sparse_slots=0, count=1,
               overflow=None):
        check(load().phantom_ckks_encode(self.ctx.handle, chain_index, 1 if ext else 0, values, num_values,
                                         sparse_slots, scale, count, out, overflow, stream))

    def decode(self, chain_index, plain, scale, values, stream, count=1):
        check(load().phantom_ckks_decode(self.ctx.handle, chain_index, plain, scale, count, values, stream))

    def encode_sub(self, chain_index, values, num_values, sub_slots, scale, out, stream, ext=False, count=1,
                   overflow=None):
        """compact sparse plaintexts [count][limbs][2 sub_slots] (NTT form over the subring)"""
        check(load().phantom_ckks_encode_sub(self.ctx.handle, chain_index, 1 if ext else 0, values, num_values,
                                             sub_slots, scale, count, out, overflow, stream))

    def sub_ntt(self, chain_index, sub_degree, data, stream, ext=False, inverse=False, count=1):
        check(load().phantom_sub_ntt(self.ctx.handle, chain_index, 1 if ext else 0, sub_degree, 1 if inverse else 0,
                                     data, count, stream))


class Encryptor:
    """Batched symmetric encryption / decryption on the device with explicit key material
    (phantom_encrypt_symmetric_batch and friends).  dev_sk, values, ciphertexts and plaintexts are
    device pointers; key (8 uint32 words), nonces (uint64 each) and seeds (64 bytes each) are host
    data.  Calls enqueue on `stream` and return; nothing is synchronised."""

    def __init__(self, ctx, dev_sk, key):
        import numpy as np
        self.ctx = ctx
        self.dev_sk = dev_sk
        self.key = np.ascontiguousarray(key, dtype=np.uint32)
        assert self.key.size == 8

    def chunk(self, chain_index):
        c = sz(0)
        check(load().phantom_encrypt_batch_chunk(self.ctx.handle, chain_index, ctypes.byref(c)))
        return c.value

    def sample_cbd_small(self, nonces, dev_out, stream):
        import numpy as np
        nn = np.ascontiguousarray(nonces, dtype=np.uint64)
        check(load().phantom_sample_cbd_small_batch(self.ctx.handle, self.key.ctypes.data, nn.ctypes.data, nn.size,
                                                    dev_out, stream))

    def encrypt(self, chain_index, values, num_values, scale, nonces, seeds, dev_out, stream, sparse_slots=0,
                out_stride=0, overflow=None):
        """seeds: bytes, 64 per ciphertext; len(nonces) ciphertexts"""
        import numpy as np
        nn = np.ascontiguousarray(nonces, dtype=np.uint64)
        seeds = bytes(seeds)
        assert len(seeds) == 64 * nn.size
        check(load().phantom_encrypt_symmetric_batch(self.ctx.handle, chain_index, self.dev_sk, values, num_values,
                                                     sparse_slots, scale, nn.size, self.key.ctypes.data, nn.ctypes.data,
                                                     seeds, dev_out, out_stride, overflow, stream))

    def decrypt(self, dev_in, polys, ct_limbs, limbs, count, dev_plain, stream, in_stride=0):
        check(load().phantom_decrypt_batch(self.ctx.handle, self.dev_sk, dev_in, in_stride, polys, ct_limbs, limbs,
                                           count, dev_plain, stream))

    def decrypt_decode(self, dev_in, polys, ct_limbs, limbs, count, scale, dev_values, stream, in_stride=0):
        check(load().phantom_decrypt_decode_batch(self.ctx.handle, self.dev_sk, dev_in, in_stride, polys, ct_limbs,
                                                  limbs, count, scale, dev_values, stream))


class PublicEncryptor:
    """Batched public-key encryption on the device with explicit key material
    (phantom_encrypt_asymmetric_batch and friends).  dev_pk ([2][size_QP][n], NTT form), values and
    ciphertexts are device pointers; key (8 uint32 words) and nonces (uint64 each, three per ciphertext:
    u, e0, e1) are host data.  Calls enqueue on `stream` and return; nothing is synchronised."""

    CBD, TERNARY = 1, 2

    def __init__(self, ctx, dev_pk, key):
        import numpy as np
        self.ctx = ctx
        self.dev_pk = dev_pk
        self.key = np.ascontiguousarray(key, dtype=np.uint32)
        assert self.key.size == 8

    def chunk(self, chain_index):
        c = sz(0)
        check(load().phantom_encrypt_asymmetric_batch_chunk(self.ctx.handle, chain_index, ctypes.byref(c)))
        return c.value

    def sample_small(self, kind, nonces, dev_out, stream):
        import numpy as np
        nn = np.ascontiguousarray(nonces, dtype=np.uint64)
        check(load().phantom_sample_small_batch(self.ctx.handle, kind, self.key.ctypes.data, nn.ctypes.data, nn.size,
                                                dev_out, stream))

    def encrypt(self, chain_index, values, num_values, scale, nonces, dev_out, stream, sparse_slots=0, out_stride=0,
                overflow=None):
        """nonces: three per ciphertext (u, e0, e1); len(nonces) / 3 ciphertexts"""
        import numpy as np
        nn = np.ascontiguousarray(nonces, dtype=np.uint64).reshape(-1)
        assert nn.size % 3 == 0
        check(load().phantom_encrypt_asymmetric_batch(self.ctx.handle, chain_index, self.dev_pk, values, num_values,
                                                      sparse_slots, scale, nn.size // 3, self.key.ctypes.data,
                                                      nn.ctypes.data, dev_out, out_stride, overflow, stream))


def _i32(values):
    import numpy as np
    return np.ascontiguousarray(values, dtype=np.int32)


class LtPrep:
    """The bootstrap's linear-transform diagonals built on the device (phantom_ltprep_*), and their
    host twins.  Device arguments are device pointers (complex128 data as interleaved doubles); offset
    lists, flags and shapes are host sequences / numpy int32 arrays.  A shape is the numpy int32 array
    [stride, center, D, g, b]."""

    MASK_NONE, MASK_OUT, MASK_IN = 0, 1, 2

    def __init__(self, ctx):
        self.ctx = ctx
        self.slots = ctx.n // 2

    @staticmethod
    def stage_offsets(ns, stages):
        import numpy as np
        st = _i32(stages)
        out = np.zeros(max(int(ns), 1), dtype=np.int32)
        cnt = sz(0)
        check(load().phantom_ltprep_stage_offsets(ns, st.ctypes.data, len(st), out.ctypes.data, len(out),
                                                  ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def stage_products(self, ns, inverse, stages, dev_out, dev_scratch, capacity, stream):
        st = _i32(stages)
        check(load().phantom_ltprep_stage_products(self.ctx.handle, ns, 1 if inverse else 0, st.ctypes.data, len(st),
                                                   dev_out, dev_scratch, capacity, stream))

    @staticmethod
    def stage_products_host(ns, inverse, stages):
        """(offsets, complex128 [D, ns]) of the host's boot::stage / boot::compose product"""
        import numpy as np
        st = _i32(stages)
        off = LtPrep.stage_offsets(ns, stages)
        out = np.zeros((len(off), ns), dtype=np.complex128)
        check(load().phantom_ltprep_stage_products_host(ns, 1 if inverse else 0, st.ctypes.data, len(st),
                                                        out.ctypes.data, len(off)))
        return off, out

    @staticmethod
    def presence(dev_band, ns, offsets, dev_flags, stream, const=None):
        off = _i32(offsets)
        c = complex(const) if const is not None else 1 + 0j
        check(load().phantom_ltprep_presence(dev_band, ns, off.ctypes.data, len(off), c.real, c.imag,
                                             0 if const is None else 1, dev_flags, stream))

    @staticmethod
    def lifted_offsets(offsets, flags, ns, n):
        import numpy as np
        off, fl = _i32(offsets), _i32(flags)
        out = np.zeros(2 * len(off) + 1, dtype=np.int32)
        cnt = sz(0)
        check(load().phantom_ltprep_lifted_offsets(off.ctypes.data, fl.ctypes.data, len(off), ns, n, out.ctypes.data,
                                                   len(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    @staticmethod
    def shape(n, keys, stride, dim1=0):
        import numpy as np
        k = _i32(keys)
        out = np.zeros(5, dtype=np.int32)
        check(load().phantom_ltprep_shape(n, k.ctypes.data, len(k), stride, dim1, out.ctypes.data))
        return out

    @staticmethod
    def finish(dev_band, ns, n, band_offsets, keys, shape, dev_out, stream, const=None, mask=0):
        """returns the slot u of each of the len(keys) output diagonals"""
        import numpy as np
        off, k, sh = _i32(band_offsets), _i32(keys), _i32(shape)
        slots = np.zeros(max(len(k), 1), dtype=np.int32)
        c = complex(const) if const is not None else 1 + 0j
        check(load().phantom_ltprep_finish(dev_band, ns, n, off.ctypes.data, len(off), k.ctypes.data, len(k),
                                           sh.ctypes.data, c.real, c.imag, 0 if const is None else 1, mask, dev_out,
                                           slots.ctypes.data, stream))
        return slots[:len(k)].copy()

    @staticmethod
    def finish_host(band, ns, n, band_offsets, stride, dim1=0, const=None, mask=0):
        """(shape, keys, slots, complex128 [K, n]) from a host band [D, ns]"""
        import numpy as np
        b = np.ascontiguousarray(band, dtype=np.complex128)
        off = _i32(band_offsets)
        cap = 2 * len(off) + 1
        sh = np.zeros(5, dtype=np.int32)
        keys, slots = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        out = np.zeros((cap, n), dtype=np.complex128)
        cnt = sz(0)
        c = complex(const) if const is not None else 1 + 0j
        check(load().phantom_ltprep_finish_host(b.ctypes.data, ns, n, off.ctypes.data, len(off), c.real, c.imag,
                                                0 if const is None else 1, mask, stride, dim1, sh.ctypes.data,
                                                keys.ctypes.data, slots.ctypes.data, cap, ctypes.byref(cnt),
                                                out.ctypes.data))
        K = cnt.value
        return sh, keys[:K].copy(), slots[:K].copy(), out[:K].copy()

    @staticmethod
    def dense_diagonals(dev_A, slots, scale, dev_out, dev_flags, stream):
        check(load().phantom_ltprep_dense_diagonals(dev_A, slots, scale, dev_out, dev_flags, stream))


class Conv:
    """The hoisted encrypted convolution's helpers (phantom_conv_*).  A shape is (width, slotstr,
    kernel, in_ch, out_ch); weights are float64 [K, K, in_ch, out_ch]; slot vectors are complex128
    [count, ns] with ns = (width 2^slotstr)^2, terms ordered (h, k, a, b) with b fastest."""

    @staticmethod
    def slots(width, slotstr):
        return (width << slotstr) ** 2

    @staticmethod
    def rotations(width, slotstr, kernel):
        import numpy as np
        out = np.zeros(kernel * kernel, dtype=np.int32)
        cnt = sz(0)
        check(load().phantom_conv_rotations(width, slotstr, kernel, out.ctypes.data, out.size, ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    @staticmethod
    def weight_slots_host(shape, W, first_term, count):
        import numpy as np
        width, slotstr, kernel, in_ch, out_ch = shape
        w = np.ascontiguousarray(W, dtype=np.float64)
        assert w.shape == (kernel, kernel, in_ch, out_ch)
        out = np.zeros((count, Conv.slots(width, slotstr)), dtype=np.complex128)
        check(load().phantom_conv_weight_slots_host(width, slotstr, kernel, in_ch, out_ch, w.ctypes.data, first_term,
                                                    count, out.ctypes.data))
        return out

    @staticmethod
    def weight_slots(shape, dev_W, first_term, count, dev_out, stream):
        width, slotstr, kernel, in_ch, out_ch = shape
        check(load().phantom_conv_weight_slots(width, slotstr, kernel, in_ch, out_ch, dev_W, first_term, count,
                                               dev_out, stream))

    @staticmethod
    def prepare(ctx, chain_index, shape, dev_W, pt_scale, stream, overflow=None):
        """a ConvPlan: the layer's weights encoded once in the compact subring form, kept on the device"""
        width, slotstr, kernel, in_ch, out_ch = shape
        h = vp()
        check(load().phantom_conv2d_prepare(ctx.handle, chain_index, in_ch, out_ch, width, slotstr, kernel, dev_W,
                                            pt_scale, overflow, stream, ctypes.byref(h)))
        return ConvPlan(h, shape)

    @staticmethod
    def prepare_scaled(ctx, chain_index, shape, dev_W, out_scale, pt_scale, stream, overflow=None):
        """prepare with output channel h's weights multiplied by out_scale[h] (host float64 [out_ch], or
        None) in FP64 on the device before the encode"""
        import numpy as np
        width, slotstr, kernel, in_ch, out_ch = shape
        sc = None
        if out_scale is not None:
            sc = np.ascontiguousarray(out_scale, dtype=np.float64)
            assert sc.shape == (out_ch,)
        h = vp()
        check(load().phantom_conv2d_prepare_scaled(ctx.handle, chain_index, in_ch, out_ch, width, slotstr, kernel, dev_W,
                                                   sc.ctypes.data if sc is not None else None, pt_scale, overflow,
                                                   stream, ctypes.byref(h)))
        return ConvPlan(h, shape)

    @staticmethod
    def apply_seeded(ctx, plan, cts, key_digits, dnum, galois_elts, outs, res, res_mult, bias, stream):
        """apply plus m res_h + B_h: res a ctypes array of out_ch device pointers (entries may be NULL) or
        None, res_mult a uint64 array [Ql] (m mod q_l), bias a uint64 array [out_ch, Ql] or None"""
        check(load().phantom_conv2d_apply_seeded(ctx.handle, plan.handle, cts, key_digits, dnum, galois_elts, outs, res,
                                                 res_mult.ctypes.data if res_mult is not None else None,
                                                 bias.ctypes.data if bias is not None else None, stream))

    @staticmethod
    def apply(ctx, plan, cts, key_digits, dnum, galois_elts, outs, stream):
        """cts / outs: ctypes arrays of device pointers; key_digits: array of K^2 arrays of dnum device
        pointers (NULL at the centre tap); galois_elts: ctypes uint32 array"""
        check(load().phantom_conv2d_apply(ctx.handle, plan.handle, cts, key_digits, dnum, galois_elts, outs, stream))


class ConvPlan:
    """Owning handle of a phantom_conv_plan (a device allocation of the layer's compact plaintexts):
    close() it, or use it as a context manager.  No apply may be in flight when it is closed."""

    def __init__(self, handle, shape):
        self.handle = handle
        self.shape = shape

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may be gone
            pass

    @property
    def bytes(self):
        b = sz(0)
        check(load().phantom_conv_plan_bytes(self.handle, ctypes.byref(b)))
        return b.value

    def words(self):
        """the plan's plaintext words [terms][Ql + P][2 ns] on the host (waits for the device)"""
        import numpy as np
        out = np.zeros(self.bytes // 8, dtype=np.uint64)
        check(load().phantom_conv_plan_read(self.handle, out.ctypes.data, out.size))
        return out

    def close(self):
        if self.handle:
            load().phantom_conv_plan_destroy(self.handle)
            self.handle = None


def ptr_array(ptrs):
    return (vp * len(ptrs))(*ptrs)


def rotate_fused_batch_chunk(ctx, chain_index):
    """ciphertexts of one chunk of rotate_fused_batch at chain_index (host only)"""
    c = sz(0)
    check(load().phantom_rotate_fused_batch_chunk(ctx.handle, chain_index, ctypes.byref(c)))
    return c.value


def rotate_fused_batch(ctx, chain_index, cts, key_digits, dnum, galois_elt, outs, stream):
    """every ciphertext of cts ([2][Ql][n] device pointers) rotated under one key into outs: sequences of
    device pointers (or ctypes arrays of them); key_digits: ctypes array of dnum device pointers"""
    assert len(cts) == len(outs)
    a = cts if isinstance(cts, ctypes.Array) else ptr_array(list(cts))
    o = outs if isinstance(outs, ctypes.Array) else ptr_array(list(outs))
    check(load().phantom_rotate_fused_batch(ctx.handle, chain_index, len(cts), a, key_digits, dnum, galois_elt, o,
                                            stream))


def keyswitch_rotate_many(ctx, chain_index, cts, digits, key_digits, dnum, galois_elt, outs, stream):
    """the batched key switch alone: outs[k] [2][Ql+P][n] from cts[k]'s c0 and digits[k] [beta][Ql+P][n],
    1 to 64 ciphertexts in one launch"""
    assert len(cts) == len(digits) == len(outs)
    check(load().phantom_keyswitch_rotate_many(ctx.handle, chain_index, len(cts), ptr_array(list(cts)),
                                               ptr_array(list(digits)), key_digits, dnum, galois_elt,
                                               ptr_array(list(outs)), stream))


class NttTables:
    """Owning handle of a phantom_ntt_tables (device NTT tables for a modulus list)."""

    def __init__(self, n, moduli):
        lib = load()
        self.n = n
        self.moduli = list(moduli)
        h = vp()
        check(lib.phantom_ntt_tables_create(n, u64_array(self.moduli), len(self.moduli), ctypes.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            load().phantom_ntt_tables_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def boot_layout(chain_index, log_n=16, depth=29, special=10, level_budget=(2, 2), num_slots=0, iterations=1):
    """(input bytes at chain_index, output bytes, output chain index) of a bootstrap session's
    serialized ciphertexts, computed on the host from the parameters (phantom_boot_layout)."""
    lb = (ctypes.c_uint32 * 2)(*level_budget)
    a, b, c = sz(0), sz(0), sz(0)
    check(load().phantom_boot_layout(log_n, depth, special, lb, num_slots, iterations, chain_index,
                                     ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


class BootSession:
    """Owning handle of a phantom_boot_session (the SimpleBootstrapExample set-up; C4/C5)."""

    def __init__(self, seed, log_n=16, depth=29, special=10, level_budget=(2, 2), num_slots=0, iterations=1,
                 precision=0, device_setup=False):
        """device_setup: build the linear-transform plaintexts on the device (off by default)"""
        lib = load()
        assert len(seed) == 32
        self.seed = bytes(seed)
        lb = (ctypes.c_uint32 * 2)(*level_budget)
        h = vp()
        check(lib.phantom_boot_session_create_opts(log_n, depth, special, lb, num_slots, iterations, precision,
                                                   self.seed, 1 if device_setup else 0, ctypes.byref(h)))
        self.device_setup = bool(device_setup)
        self.handle = h
        self.n = 1 << log_n
        self.slots = num_slots or self.n // 2
        self.depth = depth
        self.params = dict(log_n=log_n, depth=depth, special=special, level_budget=tuple(level_budget),
                           num_slots=num_slots, iterations=iterations)

    def output_bytes(self):
        b = sz(0)
        check(load().phantom_boot_output_bytes(self.handle, ctypes.byref(b)))
        return b.value

    def input_bytes(self, chain_index):
        return boot_layout(chain_index, **self.params)[0]

    def encrypt(self, values, chain_index, dev_ptr, stride):
        """values: float64 [count, slots]; writes serialized ciphertexts at dev_ptr + i * stride."""
        import numpy as np
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != self.slots:
            raise ValueError(f"values must be [count, {self.slots}], got shape {v.shape}")
        b = sz(0)
        check(load().phantom_boot_encrypt(self.handle, v.ctypes.data, v.shape[0], chain_index, dev_ptr, stride,
                                          ctypes.byref(b)))
        return b.value

    def run(self, dev_in, in_stride, count, dev_out, out_stride, lanes=4, group=None):
        """group: at most this many ciphertexts per lane in lockstep (1..8; a lane's m ciphertexts form
        ceil(m / group) groups of near-equal size); None = the library default (8)."""
        if group is None:
            check(load().phantom_boot_run(self.handle, dev_in, in_stride, count, dev_out, out_stride, lanes))
        else:
            check(load().phantom_boot_run_grouped(self.handle, dev_in, in_stride, count, dev_out, out_stride, lanes,
                                                  group))

    def decrypt(self, dev_ptr, capacity):
        import numpy as np
        out = np.zeros(self.slots, dtype=np.float64)
        check(load().phantom_boot_decrypt(self.handle, dev_ptr, capacity, out.ctypes.data))
        return out

    def encrypt_device(self, dev_values, count, chain_index, dev_ptr, stride):
        """dev_values: device complex128 [count, slots], complete when called; writes serialized
        ciphertexts at dev_ptr + i * stride and returns the size of one."""
        b = sz(0)
        check(load().phantom_boot_encrypt_device(self.handle, dev_values, count, chain_index, dev_ptr, stride,
                                                 ctypes.byref(b)))
        return b.value

    def decrypt_device(self, dev_ptr, stride, count, dev_values_out):
        """`count` serialized ciphertexts -> device complex128 [count, slots], written in the order of
        the session's stream: synchronise the device before reading them."""
        check(load().phantom_boot_decrypt_device(self.handle, dev_ptr, stride, count, dev_values_out))

    def close(self):
        if self.handle:
            load().phantom_boot_session_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pool_stats():
    """the device allocator's {held, live, peak_live, peak_held} bytes (phantom_pool_stats)"""
    out = (ctypes.c_uint64 * 4)()
    check(load().phantom_pool_stats(out))
    return dict(zip(("held", "live", "peak_live", "peak_held"), (int(x) for x in out)))


def pool_reset_peak():
    check(load().phantom_pool_reset_peak())


def traffic():
    """algorithmic bytes counted since the last reset: {"keys", "plaintexts", "ciphertexts", "total"}"""
    out = (ctypes.c_uint64 * 3)()
    check(load().phantom_traffic_read(out))
    d = {"keys": out[0], "plaintexts": out[1], "ciphertexts": out[2]}
    d["total"] = sum(d.values())
    return d


def traffic_reset():
    check(load().phantom_traffic_reset())


def bit_precision(ref, actual):
    """compute_bit_precision of bootstrapping_example.cu:17-41: mean of -log2 relative error."""
    import numpy as np
    ref = np.asarray(ref, dtype=np.float64)
    actual = np.asarray(actual, dtype=np.float64)
    keep = np.abs(ref) >= 1e-20
    rel = np.abs(ref[keep] - actual[keep]) / np.abs(ref[keep])
    rel = np.maximum(rel, 1e-40)
    return float(np.mean(-np.log2(rel))) if rel.size else 0.0
