"""LWE -> TLWE conversion and threshold partial / final decryption on the GPU: the step after the gate
path in the reference's C++ applications (src/KNN_medical_data.cpp ciphertext_conversion_threshold_decryption, src/libthfhe.cpp).
Function names and argument meaning follow the reference; samples are numpy int32 arrays, batched over the leading axis.

PackLwe is the LWE -> TLWE packing key switch (the reference's TODO at src/Convert.cpp:103): up to N samples
of any LWE dimension in ONE ring sample, so a party decrypts a 32-bit result with one partial decryption instead of 32."""
import ctypes as C

import numpy as np

from . import ThfheError, _check, _Handle, _p32, _vp, lib


class PolyContext(_Handle):
    """Device context for the ring operations (N = 1024, k = 1)."""

    def __init__(self, device=0, N=1024):
        self.N = N
        h = _vp()
        _check(lib().thfhe_poly_ctx_create(device, N, C.byref(h)))
        self._own(h, lib().thfhe_poly_ctx_destroy)
        self.pack_n = None   # LWE dimension of the packing key, once set

    def set_pack_key(self, pk, t, basebit):
        """Upload the packing key int32[n][t][2^basebit - 1][2][N] (keygen.gen_pack_key); replaces any earlier one."""
        R = (1 << basebit) - 1 if 0 < basebit < 31 else 0
        x = np.ascontiguousarray(pk, np.int32)
        row = t * R * 2 * self.N
        if R == 0 or t < 1 or x.size == 0 or x.size % row:
            raise ValueError("packing key: expected int32[n][t][2^basebit - 1][2][N]")
        _check(lib().thfhe_pack_key_set(self.h, _p32(x), x.size // row, t, basebit))
        self.pack_n = x.size // row


def TLweFromLwe(ctx, cipher):
    """src/libthfhe.cpp:340-348: LWE records int32[count][N+1] -> (a int32[count][N], b int32[count][N])."""
    x = np.ascontiguousarray(cipher, np.int32).reshape(-1, ctx.N + 1)
    a, b = np.empty((x.shape[0], ctx.N), np.int32), np.empty((x.shape[0], ctx.N), np.int32)
    _check(lib().thfhe_tlwe_from_lwe(ctx.h, _p32(x), _p32(a), _p32(b), x.shape[0]))
    return a, b


def PartialDecrypt(ctx, key_share, tlwe_a, noise=None):
    """ThFHEKeyShare::PartialDecrypt, src/libthfhe.cpp:270-293: key_share (*) a + smudging noise, exact mod 2^32."""
    s = np.ascontiguousarray(key_share, np.int32).reshape(ctx.N)
    a = np.ascontiguousarray(tlwe_a, np.int32).reshape(-1, ctx.N)
    e = np.ascontiguousarray(noise, np.int32).reshape(a.shape) if noise is not None else None
    out = np.empty_like(a)
    _check(lib().thfhe_partial_decrypt(ctx.h, _p32(s), _p32(a), _p32(e), _p32(out), a.shape[0]))
    return out


def finalDecrypt(ctx, tlwe_b, partial_ciphertexts, want_result=False):
    """src/libthfhe.cpp:296-315: b - partial_0 + sum_{i>=1} partial_i; message bit = coefficient 0 > 0."""
    b = np.ascontiguousarray(tlwe_b, np.int32).reshape(-1, ctx.N)
    parts = np.ascontiguousarray(partial_ciphertexts, np.int32).reshape(-1, b.shape[0], ctx.N)
    bits = np.empty(b.shape[0], np.int32)
    res = np.empty_like(b) if want_result else None
    _check(lib().thfhe_final_decrypt(ctx.h, _p32(b), _p32(parts), parts.shape[0], _p32(res), _p32(bits), b.shape[0]))
    return (bits.astype(bool), res) if want_result else bits.astype(bool)


def PackLwe(ctx, cipher, slots=None):
    """LWE records int32[count][n+1] (n = the packing key's dimension) -> (a, b) int32[ceil(count / slots)][N]: sample g slots + i
    lands in coefficient i of output g (slots defaults to N).  The outputs go to PartialDecrypt / finalDecrypt unchanged."""
    slots = ctx.N if slots is None else int(slots)
    if ctx.pack_n is None:
        raise ThfheError("no packing key set (PolyContext.set_pack_key)")
    x = np.ascontiguousarray(cipher, np.int32).reshape(-1, ctx.pack_n + 1)
    outs = -(-x.shape[0] // slots) if slots > 0 else 0
    a, b = np.empty((outs, ctx.N), np.int32), np.empty((outs, ctx.N), np.int32)
    if x.shape[0] == 0 and 0 < slots <= ctx.N:
        return a, b
    _check(lib().thfhe_pack_lwe(ctx.h, _p32(x), x.shape[0], slots, _p32(a), _p32(b)))
    return a, b


def PackBoxes(ctx, cipher, p):
    """thfhe_pack_boxes: LWE records int32[count][n+1], count a multiple of p -> (a, b) int32[count / p][N], one encrypted
    test vector per p samples: candidate i fills the N/p coefficients centred on i N/p (the layout of thfhe.lut.test_vector at theta = 1), ready
    for CloudKey.lut_bootstrap_enc when the packing key targets the bootstrapping ring key."""
    p = int(p)
    if ctx.pack_n is None:
        raise ThfheError("no packing key set (PolyContext.set_pack_key)")
    x = np.ascontiguousarray(cipher, np.int32).reshape(-1, ctx.pack_n + 1)
    outs = x.shape[0] // p if p > 0 else 0
    a, b = np.empty((outs, ctx.N), np.int32), np.empty((outs, ctx.N), np.int32)
    _check(lib().thfhe_pack_boxes(ctx.h, _p32(x), x.shape[0], p, _p32(a), _p32(b)))
    return a, b


def packed_bits(result, count, slots=None):
    """The message bits of `count` packed samples from finalDecrypt(..., want_result=True)'s result: coefficient i of output g is
    sample g slots + i, and its bit is that coefficient > 0."""
    res = np.asarray(result, np.int32)
    slots = res.shape[-1] if slots is None else int(slots)
    return (res.reshape(-1, res.shape[-1])[:, :slots] > 0).reshape(-1)[:count]
