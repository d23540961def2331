/* JNI glue between net.corda.core.crypto.gpu.CordaGpu (CordaGpu.kt) and libcordagpu
 * (include/cordagpu.h).  One native method per C-ABI entry point the JVM side uses:
 *
 *   nativeVerify            cg_verify_batch          Crypto.isValid / doVerify loops (Crypto.kt:472-541)
 *   nativeBatchCreate/...   cg_batch_*               a notary backlog staged once in HBM
 *   nativeTxVerify          cg_tx_verify_batch       checkSignaturesAreValid (TransactionWithSignatures.kt:58-62)
 *   nativeTxVerifyExcept    cg_tx_verify_signatures_except  verifySignaturesExcept (:41-47, 72-77)
 *   nativeFtxVerify         cg_ftx_verify_batch      FilteredTransaction.verify (MerkleTransaction.kt:173-178)
 *   nativeCompositeEval     cg_composite_eval_batch  isFulfilledBy / CompositeSignature (CompositeKey.kt:186-209)
 *   nativeSetOption         cg_set_option            a context's CORDA_AMD_* tuning knobs
 *   nativeSignerCreate/...  cg_signer_*              Ed25519 private keys expanded once on the device
 *   signBatch               cg_sign_batch            a loop of Crypto.doSign (Crypto.kt:394-401): the notary's
 *                                                    service.sign(txId.bytes) (NotaryFlow.kt:125-126)
 *   nativeEcdsaSigner...    cg_ecdsa_signer_*        EC private scalars (secp256k1 / secp256r1) held on the device
 *   ecdsaSignBatch          cg_ecdsa_sign_batch      the same doSign loop for EC keys: BC's generateSignature
 *                                                    with the nonce supplied (or RFC 6979 on the device)
 *   nativeFtxBuildLayout    cg_ftx_build_layout      output sizes of the next one (host only)
 *   buildFilteredBatch      cg_ftx_build_batch       a loop of wtx.buildFilteredTransaction (NotaryFlow.kt:72)
 *
 * Build on a JVM host against the JDK's jni.h:
 *   gcc -O2 -shared -fPIC -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -I../../include \
 *       cordagpu_jni.c -L../../corda_amd -lcordagpu -o libcordagpu_jni.so
 * (tests/native/jni_harness.c compiles it against integration/jvm/stub/jni.h and drives it
 * with a fake JNIEnv, since the image has no JDK.)
 * Every buffer is a direct ByteBuffer (little-endian for multi-byte elements): no copies,
 * no per-element JNI calls, no critical-array pin held across a multi-millisecond GPU
 * call.  A null buffer argument passes NULL (the optional outputs of the C ABI).
 * Handles: a cg_ctx* / cg_batch* as a jlong; a create call returns the handle, or the
 * (negative) cg_status when it fails. */
#include <jni.h>
#include <stdint.h>

#include "cordagpu.h"

#define CTX(h) ((cg_ctx*)(intptr_t)(h))
#define BUF(o) ((o) ? (*env)->GetDirectBufferAddress(env, (o)) : (void*)0)
#define CAP(o) ((o) ? (size_t)(*env)->GetDirectBufferCapacity(env, (o)) : (size_t)0)

JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeOpen(JNIEnv* env, jclass cls, jint device) {
  cg_ctx* ctx = 0;
  const cg_status st = cg_open((int)device, &ctx);
  return st == CG_OK ? (jlong)(intptr_t)ctx : (jlong)st;
}

JNIEXPORT void JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(JNIEnv* env, jclass cls, jlong h) {
  if (h > 0) cg_close(CTX(h));
}

JNIEXPORT jstring JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeLastError(JNIEnv* env, jclass cls, jlong h) {
  return (*env)->NewStringUTF(env, cg_last_error(h > 0 ? CTX(h) : 0));
}

/* key / value as Java Strings (value null: unset); the modified-UTF-8 bytes of an ASCII
 * option name are its C string */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeSetOption(JNIEnv* env, jclass cls, jlong h,
                                                                               jstring key, jstring value) {
  const char* k = key ? (*env)->GetStringUTFChars(env, key, 0) : 0;
  const char* v = value ? (*env)->GetStringUTFChars(env, value, 0) : 0;
  const cg_status st = cg_set_option(h > 0 ? CTX(h) : 0, k, v);
  if (v) (*env)->ReleaseStringUTFChars(env, value, v);
  if (k) (*env)->ReleaseStringUTFChars(env, key, k);
  return st;
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeVerify(
    JNIEnv* env, jclass cls, jlong h, jint n, jint mode, jobject scheme, jobject pk, jint pk_stride, jobject sig,
    jint sig_stride, jobject sig_len, jobject msg, jobject msg_off, jobject msg_len, jobject verdicts,
    jobject bitmap) {
  return cg_verify_batch(CTX(h), (size_t)n, mode, BUF(scheme), BUF(pk), (size_t)pk_stride, BUF(sig),
                         (size_t)sig_stride, BUF(sig_len), BUF(msg), CAP(msg), BUF(msg_off), BUF(msg_len),
                         BUF(verdicts), BUF(bitmap));
}

JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeBatchCreate(
    JNIEnv* env, jclass cls, jlong h, jint n, jobject scheme, jobject pk, jint pk_stride, jobject sig, jint sig_stride,
    jobject sig_len, jobject msg, jobject msg_off, jobject msg_len) {
  cg_batch* b = 0;
  const cg_status st = cg_batch_create(CTX(h), (size_t)n, BUF(scheme), BUF(pk), (size_t)pk_stride, BUF(sig),
                                       (size_t)sig_stride, BUF(sig_len), BUF(msg), CAP(msg), BUF(msg_off),
                                       BUF(msg_len), &b);
  return st == CG_OK ? (jlong)(intptr_t)b : (jlong)st;
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeBatchVerify(JNIEnv* env, jclass cls, jlong h,
                                                                              jlong batch, jint mode,
                                                                              jobject verdicts, jobject bitmap) {
  if (batch <= 0) return CG_E_INVALID_ARGUMENT;
  return cg_batch_verify(CTX(h), (cg_batch*)(intptr_t)batch, mode, BUF(verdicts), BUF(bitmap), 0);
}

JNIEXPORT void JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeBatchDestroy(JNIEnv* env, jclass cls, jlong h,
                                                                               jlong batch) {
  if (batch > 0) cg_batch_destroy(CTX(h), (cg_batch*)(intptr_t)batch);
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeTxVerify(
    JNIEnv* env, jclass cls, jlong h, jint mode, jint n_tx, jobject arena, jobject comp_off, jobject comp_len,
    jobject comp_start, jobject salts, jobject sig_start, jobject scheme, jobject pk, jint pk_stride, jobject sig,
    jint sig_stride, jobject sig_len, jobject first_bad, jobject verdicts, jobject ids) {
  return cg_tx_verify_batch(CTX(h), mode, (size_t)n_tx, BUF(arena), CAP(arena), BUF(comp_off), BUF(comp_len),
                            BUF(comp_start), BUF(salts), BUF(sig_start), BUF(scheme), BUF(pk), (size_t)pk_stride,
                            BUF(sig), (size_t)sig_stride, BUF(sig_len), BUF(first_bad), BUF(verdicts), BUF(ids));
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeTxVerifyExcept(
    JNIEnv* env, jclass cls, jlong h, jint mode, jint n_tx, jobject arena, jobject comp_off, jobject comp_len,
    jobject comp_start, jobject salts, jobject sig_start, jobject scheme, jobject pk, jint pk_stride, jobject sig,
    jint sig_stride, jobject sig_len, jobject req_start, jobject prog_start, jobject prog, jobject allowed,
    jobject status, jobject missing, jobject ids) {
  return cg_tx_verify_signatures_except(CTX(h), mode, (size_t)n_tx, BUF(arena), CAP(arena), BUF(comp_off),
                                        BUF(comp_len), BUF(comp_start), BUF(salts), BUF(sig_start), BUF(scheme),
                                        BUF(pk), (size_t)pk_stride, BUF(sig), (size_t)sig_stride, BUF(sig_len),
                                        BUF(req_start), BUF(prog_start), BUF(prog), BUF(allowed), BUF(status),
                                        BUF(missing), BUF(ids));
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxVerify(
    JNIEnv* env, jclass cls, jlong h, jint n_ftx, jobject arena, jobject comp_off, jobject comp_len,
    jobject comp_start, jobject nonces, jobject node_start, jobject node_kind, jobject node_hash, jobject roots,
    jobject result) {
  return cg_ftx_verify_batch(CTX(h), (size_t)n_ftx, BUF(arena), CAP(arena), BUF(comp_off), BUF(comp_len),
                             BUF(comp_start), BUF(nonces), BUF(node_start), BUF(node_kind), BUF(node_hash),
                             BUF(roots), BUF(result));
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeCompositeEval(
    JNIEnv* env, jclass cls, jlong h, jint n_q, jobject prog_start, jobject prog, jint n_sig, jobject sig_start,
    jobject verdicts, jobject out) {
  return cg_composite_eval_batch(CTX(h), (size_t)n_q, BUF(prog_start), BUF(prog), (size_t)n_sig, BUF(sig_start),
                                 BUF(verdicts), BUF(out));
}

/* Signing (cg_signer_*, cg_sign_batch: Crypto.doSign, Crypto.kt:394-401).  The signer handle
 * is a cg_signer* as a jlong (a failed create returns the negative cg_status); seeds: a
 * direct buffer of 32 bytes per key, which the caller overwrites after the call. */
JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerCreate(JNIEnv* env, jclass cls, jlong h,
                                                                                   jint n_keys, jobject seeds) {
  cg_signer* s = 0;
  if (n_keys < 0 || CAP(seeds) < (size_t)n_keys * 32) return CG_E_INVALID_ARGUMENT;
  const cg_status st = cg_signer_create(h > 0 ? CTX(h) : 0, (size_t)n_keys, BUF(seeds), &s);
  return st == CG_OK ? (jlong)(intptr_t)s : (jlong)st;
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerPublicKeys(JNIEnv* env, jclass cls,
                                                                                      jlong h, jlong signer,
                                                                                      jobject pk_out) {
  if (signer <= 0) return CG_E_INVALID_ARGUMENT;
  const cg_signer* s = (const cg_signer*)(intptr_t)signer;
  if (CAP(pk_out) < cg_signer_size(s) * 32) return CG_E_INVALID_ARGUMENT;
  return cg_signer_public_keys(h > 0 ? CTX(h) : 0, s, BUF(pk_out));
}

JNIEXPORT void JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerDestroy(JNIEnv* env, jclass cls, jlong h,
                                                                                   jlong signer) {
  if (h > 0 && signer > 0) cg_signer_destroy(CTX(h), (cg_signer*)(intptr_t)signer);
}

/* One call per batch: key_index (null: key 0), the message arena with its offsets and
 * lengths, sig_out (n * 64 bytes) and status (null, or n bytes) are direct buffers. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(JNIEnv* env, jclass cls, jlong h,
                                                                         jlong signer, jint n, jobject key_index,
                                                                         jobject msg, jobject msg_off,
                                                                         jobject msg_len, jobject sig_out,
                                                                         jobject status) {
  if (signer <= 0 || n < 0) return CG_E_INVALID_ARGUMENT;
  const size_t m = (size_t)n;
  if ((key_index && CAP(key_index) < 4 * m) || CAP(msg_off) < 8 * m || CAP(msg_len) < 4 * m ||
      CAP(sig_out) < 64 * m || (status && CAP(status) < m))
    return CG_E_INVALID_ARGUMENT;
  return cg_sign_batch(h > 0 ? CTX(h) : 0, (const cg_signer*)(intptr_t)signer, m, BUF(key_index), BUF(msg), CAP(msg),
                       BUF(msg_off), BUF(msg_len), BUF(sig_out), BUF(status));
}

/* FilteredTransaction construction (cg_ftx_build_layout, cg_ftx_build_batch:
 * wtx.buildFilteredTransaction, MerkleTransaction.kt:159-166 -> PartialMerkleTree.kt:66-123).
 * The layout call needs no context: it sizes the output buffers from the component counts
 * and the include mask (one byte per component).  Every buffer's capacity is checked against
 * n_tx before a start array is read. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(JNIEnv* env, jclass cls,
                                                                                    jint n_tx, jobject comp_start,
                                                                                    jobject include,
                                                                                    jobject fcomp_start,
                                                                                    jobject node_start) {
  if (n_tx < 0) return CG_E_INVALID_ARGUMENT;
  const size_t m = (size_t)n_tx;
  if (CAP(comp_start) < 4 * (m + 1) || CAP(fcomp_start) < 4 * (m + 1) || CAP(node_start) < 4 * (m + 1))
    return CG_E_INVALID_ARGUMENT;
  const uint32_t* cs = (const uint32_t*)BUF(comp_start);
  if (CAP(include) < cs[m]) return CG_E_INVALID_ARGUMENT;
  return cg_ftx_build_layout(m, cs, BUF(include), BUF(fcomp_start), BUF(node_start));
}

/* One call per batch.  The capacities handed to the library are what the output buffers
 * hold: filtered components = min(fcomp_index / 4, nonces / 32), nodes = min(node_kind,
 * node_hash / 32); too small comes back as CG_E_INVALID_ARGUMENT with the needed counts in
 * nativeLastError. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(
    JNIEnv* env, jclass cls, jlong h, jint n_tx, jobject arena, jobject comp_off, jobject comp_len, jobject comp_start,
    jobject salts, jobject include, jobject fcomp_start, jobject fcomp_index, jobject nonces, jobject node_start,
    jobject node_kind, jobject node_hash, jobject roots) {
  if (n_tx < 0) return CG_E_INVALID_ARGUMENT;
  const size_t m = (size_t)n_tx;
  if (CAP(comp_start) < 4 * (m + 1) || CAP(fcomp_start) < 4 * (m + 1) || CAP(node_start) < 4 * (m + 1) ||
      CAP(salts) < 32 * m || CAP(roots) < 32 * m)
    return CG_E_INVALID_ARGUMENT;
  const size_t n_comp = ((const uint32_t*)BUF(comp_start))[m];
  if (CAP(include) < n_comp || CAP(comp_off) < 8 * n_comp || CAP(comp_len) < 4 * n_comp) return CG_E_INVALID_ARGUMENT;
  size_t fcap = CAP(fcomp_index) / 4, ncap = CAP(node_kind);
  if (CAP(nonces) / 32 < fcap) fcap = CAP(nonces) / 32;
  if (CAP(node_hash) / 32 < ncap) ncap = CAP(node_hash) / 32;
  return cg_ftx_build_batch(h > 0 ? CTX(h) : 0, m, BUF(arena), CAP(arena), BUF(comp_off), BUF(comp_len),
                            BUF(comp_start), BUF(salts), BUF(include), fcap, ncap, BUF(fcomp_start), BUF(fcomp_index),
                            BUF(nonces), BUF(node_start), BUF(node_kind), BUF(node_hash), BUF(roots));
}

/* ECDSA signing (cg_ecdsa_signer_*, cg_ecdsa_sign_batch: Crypto.doSign for an EC private key).
 * The signer handle is a cg_ecdsa_signer* as a jlong (a failed create returns the negative
 * cg_status); d: a direct buffer of 32 big-endian bytes per key, which the caller overwrites
 * after the call. */
JNIEXPORT jlong JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(JNIEnv* env, jclass cls,
                                                                                        jlong h, jint scheme,
                                                                                        jint n_keys, jobject d) {
  cg_ecdsa_signer* s = 0;
  if (n_keys < 0 || CAP(d) < (size_t)n_keys * 32) return CG_E_INVALID_ARGUMENT;
  const cg_status st = cg_ecdsa_signer_create(h > 0 ? CTX(h) : 0, scheme, (size_t)n_keys, BUF(d), &s);
  return st == CG_OK ? (jlong)(intptr_t)s : (jlong)st;
}

JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerPublicKeys(JNIEnv* env, jclass cls,
                                                                                           jlong h, jlong signer,
                                                                                           jobject xy_out) {
  if (signer <= 0) return CG_E_INVALID_ARGUMENT;
  const cg_ecdsa_signer* s = (const cg_ecdsa_signer*)(intptr_t)signer;
  if (CAP(xy_out) < cg_ecdsa_signer_size(s) * 64) return CG_E_INVALID_ARGUMENT;
  return cg_ecdsa_signer_public_keys(h > 0 ? CTX(h) : 0, s, BUF(xy_out));
}

JNIEXPORT void JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerDestroy(JNIEnv* env, jclass cls,
                                                                                        jlong h, jlong signer) {
  if (h > 0 && signer > 0) cg_ecdsa_signer_destroy(CTX(h), (cg_ecdsa_signer*)(intptr_t)signer);
}

/* One call per batch: key_index (null: key 0), the message arena with its offsets and lengths,
 * k_be (n * 32 bytes; null in RFC 6979 mode), sig_out (n * sig_stride bytes), sig_len_out
 * (n * 4 bytes) and status (null, or n bytes) are direct buffers. */
JNIEXPORT jint JNICALL Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(
    JNIEnv* env, jclass cls, jlong h, jlong signer, jint n, jobject key_index, jobject msg, jobject msg_off,
    jobject msg_len, jint nonce_mode, jobject k_be, jobject sig_out, jint sig_stride, jobject sig_len_out,
    jobject status) {
  if (signer <= 0 || n < 0 || sig_stride < 0) return CG_E_INVALID_ARGUMENT;
  const size_t m = (size_t)n;
  if ((key_index && CAP(key_index) < 4 * m) || CAP(msg_off) < 8 * m || CAP(msg_len) < 4 * m ||
      (k_be && CAP(k_be) < 32 * m) || CAP(sig_out) < (size_t)sig_stride * m || CAP(sig_len_out) < 4 * m ||
      (status && CAP(status) < m))
    return CG_E_INVALID_ARGUMENT;
  return cg_ecdsa_sign_batch(h > 0 ? CTX(h) : 0, (const cg_ecdsa_signer*)(intptr_t)signer, m, BUF(key_index), BUF(msg),
                             CAP(msg), BUF(msg_off), BUF(msg_len), nonce_mode, BUF(k_be), BUF(sig_out),
                             (size_t)sig_stride, BUF(sig_len_out), BUF(status));
}
