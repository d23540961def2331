"""Batch signature verification surface mirroring Corda's ``Crypto`` object.

Reference (Kerwong/corda @ 0.14):
  * ``Crypto.isValid(scheme, publicKey, signatureData, clearData)``
    core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:534-541
  * ``Crypto.doVerify(scheme, publicKey, signatureData, clearData)``
    Crypto.kt:472-483 (empty sig / data -> IllegalArgumentException; ``false`` ->
    SignatureException("Signature Verification failed!"))
  * schemes ``ECDSA_SECP256K1_SHA256`` (2), ``ECDSA_SECP256R1_SHA256`` (3),
    ``EDDSA_ED25519_SHA512`` (4) — Crypto.kt:91-132

``is_valid_batch`` returns one verdict code per element (what a loop of
``isValid`` would have returned / thrown); ``do_verify_batch`` raises exactly the
exception a ``for`` loop over ``doVerify`` would raise first (lowest failing
index), so callers such as ``checkSignaturesAreValid`` keep their semantics.
The work runs in libcordagpu's HIP kernels; this module only marshals buffers.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import ACCEPT, ARG_EMPTY, KEY_INVALID, MODE_DO_VERIFY, MODE_IS_VALID, REJECT, SIG_MALFORMED, UNSUPPORTED


@dataclass(frozen=True)
class SignatureScheme:
    """Subset of ``net.corda.core.crypto.SignatureScheme`` (SignatureScheme.kt:22-32)."""

    scheme_number_id: int
    scheme_code_name: str
    signature_name: str


ECDSA_SECP256K1_SHA256 = SignatureScheme(2, "ECDSA_SECP256K1_SHA256", "SHA256withECDSA")
ECDSA_SECP256R1_SHA256 = SignatureScheme(3, "ECDSA_SECP256R1_SHA256", "SHA256withECDSA")
EDDSA_ED25519_SHA512 = SignatureScheme(4, "EDDSA_ED25519_SHA512", "NONEwithEdDSA")
SUPPORTED_SCHEMES = {s.scheme_code_name: s for s in (ECDSA_SECP256K1_SHA256, ECDSA_SECP256R1_SHA256,
                                                      EDDSA_ED25519_SHA512)}


class IllegalArgumentException(ValueError):
    """java.lang.IllegalArgumentException raised by the reference (e.g. Crypto.kt:475-476)."""

    def __init__(self, msg: str, index: int | None = None):
        super().__init__(msg)
        self.index = index


class SignatureException(Exception):
    """java.security.SignatureException (Crypto.kt:481, or a malformed signature in the engine)."""

    def __init__(self, msg: str, index: int | None = None):
        super().__init__(msg)
        self.index = index


class InvalidKeyException(Exception):
    """java.security.InvalidKeyException: the public key cannot be used."""

    def __init__(self, msg: str, index: int | None = None):
        super().__init__(msg)
        self.index = index


def _scheme_id(s) -> int:
    if isinstance(s, SignatureScheme):
        return s.scheme_number_id
    if isinstance(s, str):
        if s not in SUPPORTED_SCHEMES:
            raise IllegalArgumentException(f"Unsupported key/algorithm for schemeCodeName: {s}")
        return SUPPORTED_SCHEMES[s].scheme_number_id
    return int(s)


KEY_BYTES = {ECDSA_SECP256K1_SHA256.scheme_number_id: 64, ECDSA_SECP256R1_SHA256.scheme_number_id: 64,
             EDDSA_ED25519_SHA512.scheme_number_id: 32}


def key_length_ok(scheme_id: int, key) -> bool:
    """The key bytes must be the scheme's wire form: 32-byte A for Ed25519 (i2p's
    EdDSAPublicKeySpec refuses any other length, so the key object cannot exist),
    64-byte X||Y for ECDSA (see corda_amd.keys for X.509 decoding).  Keys are never
    truncated or zero-padded into that form."""
    want = KEY_BYTES.get(scheme_id)
    return want is None or len(bytes(key)) == want


# OR-ed into the scheme id of an element whose key bytes are not the scheme's wire form
# (include/cordagpu.h CG_SCHEME_FLAG_KEY_INVALID): the key object cannot be constructed,
# so the library reports KEY_INVALID for it on every path (verify, prepared batches and
# their device bitmaps, shards, transactions) and never reads its rows.
SCHEME_FLAG_KEY_INVALID = 0x80


def pack_key_row(pk: np.ndarray, scheme: np.ndarray, i: int, key) -> bool:
    """Writes element i's key row (device schemes only — the rows of host-verified schemes
    such as RSA are never read by the device and may be any length).  A key of the wrong
    length flags the element KEY_INVALID and leaves its row zero.  Returns False for it."""
    sid = int(scheme[i])
    if sid not in KEY_BYTES:
        return True
    kb = bytes(key)
    if not key_length_ok(sid, kb):
        scheme[i] = sid | SCHEME_FLAG_KEY_INVALID
        return False
    pk[i, :len(kb)] = np.frombuffer(kb, dtype=np.uint8)
    return True


@dataclass
class PackedBatch:
    """Element-major host buffers in the C ABI's layout."""

    n: int
    scheme: np.ndarray
    pk: np.ndarray
    pk_stride: int
    sig: np.ndarray
    sig_stride: int
    sig_len: np.ndarray
    msg: np.ndarray
    msg_off: np.ndarray
    msg_len: np.ndarray
    # elements whose key bytes are not the scheme's wire form (flagged in `scheme` with
    # SCHEME_FLAG_KEY_INVALID: the library gives them KEY_INVALID); informational
    key_invalid: np.ndarray | None = None


def pack(schemes, public_keys: Sequence[bytes], signatures: Sequence[bytes], clear_data: Sequence[bytes]) -> PackedBatch:
    """Packs per-element byte strings.  ``public_keys``: Ed25519 32-byte A, ECDSA
    64-byte X||Y (see corda_amd.keys for X.509 decoding).  ``schemes`` may be a
    single scheme or one per element."""
    n = len(signatures)
    if not (len(public_keys) == n == len(clear_data)):
        raise IllegalArgumentException("public_keys, signatures and clear_data differ in length")
    if isinstance(schemes, (SignatureScheme, str, int)):
        scheme = np.full(n, _scheme_id(schemes), dtype=np.uint8)
    else:
        scheme = np.array([_scheme_id(s) for s in schemes], dtype=np.uint8)
    pk_stride = 64
    pk = np.zeros((max(n, 1), pk_stride), dtype=np.uint8)
    bad_keys = [i for i, k in enumerate(public_keys) if not pack_key_row(pk, scheme, i, k)]
    maxlen = max([len(s) for s in signatures] + [64])
    sig_stride = (maxlen + 3) // 4 * 4
    sig = np.zeros((max(n, 1), sig_stride), dtype=np.uint8)
    sig_len = np.zeros(max(n, 1), dtype=np.uint32)
    for i, s in enumerate(signatures):
        sb = bytes(s)
        sig[i, :len(sb)] = np.frombuffer(sb, dtype=np.uint8)
        sig_len[i] = len(sb)
    msg_len = np.array([len(m) for m in clear_data] + [0] * (n == 0), dtype=np.uint32)
    msg_off = np.zeros(max(n, 1), dtype=np.uint64)
    if n:
        msg_off[1:n] = np.cumsum(msg_len[:n - 1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(bytes(m) for m in clear_data) or b"\0", dtype=np.uint8).copy()
    return PackedBatch(n, scheme, pk, pk_stride, sig, sig_stride, sig_len, arena, msg_off, msg_len,
                       np.array(bad_keys, dtype=np.int64) if bad_keys else None)


def verify_packed(ctx: _lib.Context, b: PackedBatch, mode: int, bitmap: bool = False):
    verdict = np.empty(max(b.n, 1), dtype=np.uint8)
    bm = np.zeros(max((b.n + 31) // 32, 1), dtype=np.uint32) if bitmap else None
    ctx.check(ctx.lib.cg_verify_batch(ctx.h, b.n, mode, _lib.ptr(b.scheme), _lib.ptr(b.pk), b.pk_stride,
                                      _lib.ptr(b.sig), b.sig_stride, _lib.ptr(b.sig_len), _lib.ptr(b.msg),
                                      len(b.msg), _lib.ptr(b.msg_off), _lib.ptr(b.msg_len), _lib.ptr(verdict),
                                      _lib.ptr(bm)))
    return (verdict[:b.n], bm) if bitmap else verdict[:b.n]


# Schemes Crypto supports (Crypto.kt:176-183) that the device does not run: RSA_SHA256 (1),
# SPHINCS-256_SHA512 (5) and COMPOSITE (6) are verified by the host's own JCA path.
HOST_SCHEMES = {1: "RSA_SHA256", 5: "SPHINCS-256_SHA512", 6: "COMPOSITE"}


def _verify_mixed(ctx, schemes, public_keys, signatures, clear_data, mode, host_verify):
    """Device batch for schemes 2/3/4; elements of HOST_SCHEMES go to
    ``host_verify(scheme_id, key, signature, data, mode) -> verdict code`` (on the JVM:
    Crypto.isValid / doVerify under try/catch) and are merged back in index order, so
    first-failure-wins still holds.  Without a host_verifier such elements raise
    IllegalArgumentException — they are not silently reported UNSUPPORTED."""
    b = pack(schemes, public_keys, signatures, clear_data)
    host = np.flatnonzero(np.isin(b.scheme[:b.n], list(HOST_SCHEMES)))
    if host.size and host_verify is None:
        i = int(host[0])
        raise IllegalArgumentException(f"scheme {HOST_SCHEMES[int(b.scheme[i])]} is verified on the host JCA path: "
                                       "pass host_verify", i)
    v = verify_packed(ctx, b, mode)
    for i in host:
        i = int(i)
        v[i] = host_verify(int(b.scheme[i]), bytes(public_keys[i]), bytes(signatures[i]), bytes(clear_data[i]), mode)
    return v


def is_valid_batch(ctx: _lib.Context, schemes, public_keys, signatures, clear_data, host_verify=None) -> np.ndarray:
    """Per-element verdict codes of ``Crypto.isValid`` (ACCEPT=0 means ``true``,
    REJECT=1 ``false``; 2/3/5 mean isValid would have thrown)."""
    return _verify_mixed(ctx, schemes, public_keys, signatures, clear_data, MODE_IS_VALID, host_verify)


def raise_for_verdict(code: int, index: int):
    """The exception ``Crypto.doVerify`` throws for a non-ACCEPT verdict."""
    if code == REJECT:
        raise SignatureException("Signature Verification failed!", index)
    if code == SIG_MALFORMED:
        raise SignatureException("signature length is wrong / error decoding signature bytes.", index)
    if code == KEY_INVALID:
        raise InvalidKeyException("public key cannot be decoded", index)
    if code == ARG_EMPTY:
        raise IllegalArgumentException("Signature data is empty! / Clear data is empty, nothing to verify!", index)
    if code == UNSUPPORTED:
        raise IllegalArgumentException("Unsupported key/algorithm", index)


def do_verify_batch(ctx: _lib.Context, schemes, public_keys, signatures, clear_data, host_verify=None) -> bool:
    """``for i in range(n): Crypto.doVerify(...)``: returns True or raises the
    exception of the lowest failing index."""
    v = _verify_mixed(ctx, schemes, public_keys, signatures, clear_data, MODE_DO_VERIFY, host_verify)
    bad = np.flatnonzero(v != ACCEPT)
    if bad.size:
        i = int(bad[0])
        raise_for_verdict(int(v[i]), i)
    return True


class PreparedBatch:
    """A batch staged once in HBM (``cg_batch_create``) and verified on demand."""

    def __init__(self, ctx: _lib.Context, b: PackedBatch):
        self.ctx, self.n = ctx, b.n
        h = _lib.c_void_p()
        ctx.check(ctx.lib.cg_batch_create(ctx.h, b.n, _lib.ptr(b.scheme), _lib.ptr(b.pk), b.pk_stride,
                                          _lib.ptr(b.sig), b.sig_stride, _lib.ptr(b.sig_len), _lib.ptr(b.msg),
                                          len(b.msg), _lib.ptr(b.msg_off), _lib.ptr(b.msg_len),
                                          _lib.ctypes.byref(h)))
        self.h = h

    def verify(self, mode: int = MODE_IS_VALID, want_verdicts: bool = True, device_bitmap_ptr: int | None = None):
        verdict = np.empty(max(self.n, 1), dtype=np.uint8) if want_verdicts else None
        self.ctx.check(self.ctx.lib.cg_batch_verify(self.ctx.h, self.h, mode, _lib.ptr(verdict), None,
                                                    device_bitmap_ptr))
        return verdict[:self.n] if want_verdicts else None

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.cg_batch_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------- signing
# ``Crypto.doSign(privateKey, clearData)`` (Crypto.kt:394-401) for EDDSA_ED25519_SHA512
# keys, batched: what a notary does to every transaction id it accepts
# (NotaryFlow.kt:125-126 -> NotaryService.kt:75-77 -> keyManagementService.sign).  i2p's
# EdDSAEngine signs deterministically (RFC 8032), so the 64 bytes equal the JVM's.  EC keys
# sign through EcdsaSigner / ecdsa_sign_batch: BC's ECDSASigner.generateSignature is a pure
# function of (d, e, k), so with the nonce k given by the caller (drawn as BC draws it) the DER
# bytes equal BC's, and with RFC 6979 nonces derived on the device no randomness is needed.
SIGN_OK, SIGN_EMPTY = _lib.SIGN_OK, _lib.SIGN_EMPTY


class SigningException(Exception):
    """What ``Crypto.doSign`` throws for an element (Crypto.kt:397: empty clear data), or a
    signature that failed its verify-after-sign check."""

    def __init__(self, msg: str, index: int | None = None):
        super().__init__(msg)
        self.index = index


def entropy_to_seed(k: int) -> bytes:
    """The Ed25519 seed of Corda's ``entropyToKeyPair(BigInteger.valueOf(k))``
    (Crypto.kt:733-739): ``BigInteger.toByteArray()`` (big-endian, minimal two's
    complement) then ``copyOf(32)`` (cut or zero-padded on the right to 32 bytes)."""
    raw = int(k).to_bytes((int(k).bit_length() + 8) // 8, "big", signed=True)
    return (raw + bytes(32))[:32]


class Ed25519Signer:
    """Private keys held on the device (``cg_signer_create``).  ``seeds``: one 32-byte seed
    per key, the wire form of an ``EdDSAPrivateKey`` (Kryo.kt:316-320)."""

    def __init__(self, ctx: _lib.Context, seeds: Sequence[bytes]):
        seeds = [bytes(s) for s in seeds]
        if any(len(s) != 32 for s in seeds):
            raise IllegalArgumentException("an Ed25519 seed is 32 bytes")
        self.ctx, self.n_keys, self.h = ctx, len(seeds), None
        buf = np.frombuffer(b"".join(seeds) or bytes(32), dtype=np.uint8).copy()
        h = _lib.c_void_p()
        try:
            ctx.check(ctx.lib.cg_signer_create(ctx.h, self.n_keys, _lib.ptr(buf), _lib.ctypes.byref(h)))
        finally:
            buf[:] = 0  # this module's own copy of the seeds
        self.h = h
        self._pk = None

    @property
    def public_keys(self) -> list[bytes]:
        if self._pk is None:
            out = np.zeros((max(self.n_keys, 1), 32), dtype=np.uint8)
            self.ctx.check(self.ctx.lib.cg_signer_public_keys(self.ctx.h, self.h, _lib.ptr(out)))
            self._pk = [out[j].tobytes() for j in range(self.n_keys)]
        return list(self._pk)

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:  # (a closed context has already released the device arrays)
                self.ctx.lib.cg_signer_destroy(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sign_packed(ctx: _lib.Context, signer: Ed25519Signer, msg: np.ndarray, msg_off: np.ndarray, msg_len: np.ndarray,
                key_index: np.ndarray | None = None):
    """``cg_sign_batch`` on arrays in the C ABI's layout (the message arena of
    ``PackedBatch``); returns (signatures [n, 64] uint8, status [n] uint8)."""
    n = len(msg_len)
    msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64)
    msg_len = np.ascontiguousarray(msg_len, dtype=np.uint32)
    if key_index is not None:
        key_index = np.ascontiguousarray(key_index, dtype=np.uint32)
        if len(key_index) != n:
            raise IllegalArgumentException("key_index and clear_data differ in length")
    if len(msg_off) != n:
        raise IllegalArgumentException("msg_off and msg_len differ in length")
    sig = np.zeros((max(n, 1), 64), dtype=np.uint8)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    ctx.check(ctx.lib.cg_sign_batch(ctx.h, signer.h, n, _lib.ptr(key_index), _lib.ptr(msg), len(msg),
                                    _lib.ptr(msg_off), _lib.ptr(msg_len), _lib.ptr(sig), _lib.ptr(status)))
    return sig[:n], status[:n]


def sign_batch(ctx: _lib.Context, signer: Ed25519Signer, clear_data: Sequence[bytes], key_index=None):
    """Signs clear_data[i] with key key_index[i] of the signer (None: key 0 throughout).
    Returns (signatures [n, 64] uint8, status [n]): SIGN_OK, or SIGN_EMPTY with a zero row
    for empty clear data."""
    n = len(clear_data)
    msg_len = np.array([len(m) for m in clear_data], dtype=np.uint32)
    msg_off = np.zeros(n, dtype=np.uint64)
    if n:
        msg_off[1:] = np.cumsum(msg_len[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(bytes(m) for m in clear_data) or b"\0", dtype=np.uint8).copy()
    return sign_packed(ctx, signer, arena, msg_off, msg_len, key_index)


class EcdsaSigner:
    """EC private keys of one curve held on the device (``cg_ecdsa_signer_create``).
    ``scheme``: ECDSA_SECP256K1_SHA256 or ECDSA_SECP256R1_SHA256 (or its id 2 / 3);
    ``private_scalars``: d per key as an int or as 32 big-endian bytes, 0 < d < n."""

    def __init__(self, ctx: _lib.Context, scheme, private_scalars: Sequence):
        self.scheme = _scheme_id(scheme)
        rows = [int(d).to_bytes(32, "big") if isinstance(d, int) else bytes(d) for d in private_scalars]
        if any(len(r) != 32 for r in rows):
            raise IllegalArgumentException("an EC private scalar is 32 big-endian bytes")
        self.ctx, self.n_keys, self.h = ctx, len(rows), None
        buf = np.frombuffer(b"".join(rows) or bytes(32), dtype=np.uint8).copy()
        h = _lib.c_void_p()
        try:
            ctx.check(ctx.lib.cg_ecdsa_signer_create(ctx.h, self.scheme, self.n_keys, _lib.ptr(buf),
                                                     _lib.ctypes.byref(h)))
        finally:
            buf[:] = 0  # this module's own copy of the scalars
        self.h = h
        self._pk = None

    @property
    def public_keys(self) -> list[bytes]:
        """Q = d G per key as 64 bytes X || Y: the key form ``pack`` takes for the ECDSA schemes."""
        if self._pk is None:
            out = np.zeros((max(self.n_keys, 1), 64), dtype=np.uint8)
            self.ctx.check(self.ctx.lib.cg_ecdsa_signer_public_keys(self.ctx.h, self.h, _lib.ptr(out)))
            self._pk = [out[j].tobytes() for j in range(self.n_keys)]
        return list(self._pk)

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:  # (a closed context has already released the device arrays)
                self.ctx.lib.cg_ecdsa_signer_destroy(self.ctx.h, self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SIGN_NONCE_INVALID, SIGN_DEGENERATE = _lib.SIGN_NONCE_INVALID, _lib.SIGN_DEGENERATE


def ecdsa_sign_packed(ctx: _lib.Context, signer: EcdsaSigner, msg: np.ndarray, msg_off: np.ndarray,
                      msg_len: np.ndarray, key_index: np.ndarray | None = None, nonces: np.ndarray | None = None,
                      sig_stride: int = _lib.ECDSA_SIG_MAX):
    """``cg_ecdsa_sign_batch`` on arrays in the C ABI's layout; ``nonces``: [n, 32] uint8
    big-endian rows (caller mode) or None (RFC 6979).  Returns (signatures [n, sig_stride]
    uint8, sig_len [n] uint32, status [n] uint8): the sig / sig_len arrays of ``PackedBatch``."""
    n = len(msg_len)
    msg_off = np.ascontiguousarray(msg_off, dtype=np.uint64)
    msg_len = np.ascontiguousarray(msg_len, dtype=np.uint32)
    if key_index is not None:
        key_index = np.ascontiguousarray(key_index, dtype=np.uint32)
        if len(key_index) != n:
            raise IllegalArgumentException("key_index and clear_data differ in length")
    if len(msg_off) != n:
        raise IllegalArgumentException("msg_off and msg_len differ in length")
    mode = _lib.ECDSA_NONCE_RFC6979
    if nonces is not None:
        mode = _lib.ECDSA_NONCE_CALLER
        nonces = np.ascontiguousarray(nonces, dtype=np.uint8).reshape(-1, 32)
        if len(nonces) != n:
            raise IllegalArgumentException("nonces and clear_data differ in length")
        if n == 0:
            nonces = np.zeros((1, 32), dtype=np.uint8)
    sig = np.zeros((max(n, 1), sig_stride), dtype=np.uint8)
    sig_len = np.zeros(max(n, 1), dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    ctx.check(ctx.lib.cg_ecdsa_sign_batch(ctx.h, signer.h, n, _lib.ptr(key_index), _lib.ptr(msg), len(msg),
                                          _lib.ptr(msg_off), _lib.ptr(msg_len), mode, _lib.ptr(nonces), _lib.ptr(sig),
                                          sig_stride, _lib.ptr(sig_len), _lib.ptr(status)))
    return sig[:n], sig_len[:n], status[:n]


def ecdsa_sign_batch(ctx: _lib.Context, signer: EcdsaSigner, clear_data: Sequence[bytes], key_index=None, nonces=None):
    """Signs clear_data[i] with key key_index[i] of the signer (None: key 0 throughout).
    ``nonces``: None for RFC 6979 nonces derived on the device, or one k per element (int or
    32 big-endian bytes) drawn as BC's RandomDSAKCalculator draws it.  Returns (DER signatures
    as a list of bytes, status [n]): SIGN_OK, or b"" with SIGN_EMPTY / SIGN_NONCE_INVALID /
    SIGN_DEGENERATE."""
    n = len(clear_data)
    msg_len = np.array([len(m) for m in clear_data], dtype=np.uint32)
    msg_off = np.zeros(n, dtype=np.uint64)
    if n:
        msg_off[1:] = np.cumsum(msg_len[:-1], dtype=np.uint64)
    arena = np.frombuffer(b"".join(bytes(m) for m in clear_data) or b"\0", dtype=np.uint8).copy()
    rows = None
    if nonces is not None:
        if len(nonces) != n:
            raise IllegalArgumentException("nonces and clear_data differ in length")
        rows = np.frombuffer(b"".join(int(k).to_bytes(32, "big") if isinstance(k, int) else bytes(k) for k in nonces),
                             dtype=np.uint8).copy().reshape(-1, 32) if n else np.zeros((0, 32), dtype=np.uint8)
    sig, sig_len, status = ecdsa_sign_packed(ctx, signer, arena, msg_off, msg_len, key_index, rows)
    if rows is not None:
        rows[:] = 0
    return [sig[i, :sig_len[i]].tobytes() for i in range(n)], status


_SIGN_FAILURES = {
    _lib.SIGN_EMPTY: "Signing of an empty array is not permitted!",
    _lib.SIGN_NONCE_INVALID: "the nonce is outside [1, n-1]",
    _lib.SIGN_DEGENERATE: "the nonce gives r = 0 or s = 0",
}


def do_sign_batch(ctx: _lib.Context, signer, clear_data: Sequence[bytes], key_index=None,
                  verify_after_sign: bool = False, nonces=None) -> list[bytes]:
    """``for i in range(n): Crypto.doSign(key[key_index[i]], clear_data[i])`` for an
    ``Ed25519Signer`` or an ``EcdsaSigner``: the n signatures, or the exception of the lowest
    failing index.  ``nonces`` (EcdsaSigner only): as in ``ecdsa_sign_batch``.
    verify_after_sign: every signature is verified on the device before any is returned, the
    usual guard against a faulted computation leaking the key."""
    if isinstance(signer, EcdsaSigner):
        sigs, status = ecdsa_sign_batch(ctx, signer, clear_data, key_index, nonces)
        scheme = signer.scheme
    else:
        if nonces is not None:
            raise IllegalArgumentException("nonces apply to an EcdsaSigner only")
        sig, status = sign_batch(ctx, signer, clear_data, key_index)
        sigs = [sig[i].tobytes() for i in range(len(clear_data))]
        scheme = EDDSA_ED25519_SHA512
    bad = np.flatnonzero(status != SIGN_OK)
    if bad.size:
        raise SigningException(_SIGN_FAILURES.get(int(status[bad[0]]), "signing failed"), int(bad[0]))
    if verify_after_sign and sigs:
        pks = signer.public_keys
        idx = np.zeros(len(sigs), dtype=np.int64) if key_index is None else np.asarray(key_index, dtype=np.int64)
        v = is_valid_batch(ctx, scheme, [pks[int(j)] for j in idx], sigs, clear_data)
        wrong = np.flatnonzero(v != ACCEPT)
        if wrong.size:
            raise SigningException("signature failed verification after signing", int(wrong[0]))
    return sigs
