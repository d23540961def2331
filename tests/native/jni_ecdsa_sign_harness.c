/*
 * Drives the ECDSA signing natives of integration/jvm/cordagpu_jni.c (compiled against the stub
 * jni.h) through a fake JNIEnv whose direct ByteBuffers are plain C buffers.  `cpu`: no
 * device — every native refuses a failed context or signer handle with a status, nothing
 * crashes; `gpu`: the P-256 key of RFC 6979 appendix A.2.5 signs "sample" and "test" with
 * SHA-256 in RFC 6979 mode (the appendix's r and s, as DER) beside an empty element, a
 * secp256k1 key signs with a caller nonce whose top window is all ones (expected bytes from
 * oracle/py/ecdsa_bc.py), public keys compared byte for byte, and every signature verified
 * through nativeVerify with the buffers signBatch filled.
 */
#include <stdio.h>
#include <string.h>

#include <jni.h>

#include "cordagpu.h"

struct _jobject {
  void* addr;
  jlong cap;
};

static void* buf_addr(JNIEnv* env, jobject b) { return b->addr; }
static jlong buf_cap(JNIEnv* env, jobject b) { return b->cap; }
static const char* last_string;
static jstring new_string(JNIEnv* env, const char* s) {
  last_string = s;
  return (jstring)0;
}
static const char* get_utf(JNIEnv* env, jstring s, jboolean* is_copy) { return (const char*)s; }
static void release_utf(JNIEnv* env, jstring s, const char* utf) {}
static const struct JNINativeInterface_ kIface = {buf_addr, buf_cap, new_string, get_utf, release_utf};

jlong Java_net_corda_core_crypto_gpu_CordaGpu_nativeOpen(JNIEnv*, jclass, jint);
void Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(JNIEnv*, jclass, jlong);
jstring Java_net_corda_core_crypto_gpu_CordaGpu_nativeLastError(JNIEnv*, jclass, jlong);
jint Java_net_corda_core_crypto_gpu_CordaGpu_nativeVerify(JNIEnv*, jclass, jlong, jint, jint, jobject, jobject, jint,
                                                          jobject, jint, jobject, jobject, jobject, jobject, jobject,
                                                          jobject);
jlong Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(JNIEnv*, jclass, jlong, jint, jint, jobject);
jint Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerPublicKeys(JNIEnv*, jclass, jlong, jlong, jobject);
void Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerDestroy(JNIEnv*, jclass, jlong, jlong);
jint Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(JNIEnv*, jclass, jlong, jlong, jint, jobject, jobject,
                                                            jobject, jobject, jint, jobject, jobject, jint, jobject,
                                                            jobject);

static int failures;
#define CHECK(c, m)                                       \
  do {                                                    \
    if (!(c)) {                                           \
      fprintf(stderr, "FAIL line %d: %s\n", __LINE__, m); \
      ++failures;                                         \
    }                                                     \
  } while (0)

static size_t hex(uint8_t* out, const char* h) {
  size_t i = 0;
  for (; h[2 * i]; ++i) {
    unsigned v;
    sscanf(h + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
  return i;
}

/* RFC 6979 A.2.5: the P-256 key, its public key, and the SHA-256 signatures of "sample" and "test" */
static const char* kR1d = "c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721";
static const char* kR1q =
    "60fed4ba255a9d31c961eb74c6356d68c049b8923b61fa6ce669622e60f29fb6"
    "7903fe1008b8bc99a41ae9e95628bc64f2f1b20c2d7e9f5177a3c294d4462299";
static const char* kR1sample =
    "3046022100efd48b2aacb6a8fd1140dd9cd45e81d69d2c877b56aaf991c34d0ea84eaf3716"
    "022100f7cb1c942d657c41d436c7a1b6e29f65f3e900dbb9aff4064dc4ab2f843acda8";
static const char* kR1test =
    "3045022100f1abb023518351cd71d881567b1ea663ed3efcf6c5132b354f28d3b0b7d38367"
    "0220019f4113742a2b14bd25926b49c649155f267e60d3814b4c0cc84250e46f0083";
/* secp256k1: a key, its public key, "sample" under the caller nonce kK1k, and under RFC 6979 */
static const char* kK1d = "1e99423a4ed27608a15a2616a2b0e9e52ced330ac530edcc32c8ffc6a526aedd";
static const char* kK1q =
    "f028892bad7ed57d2fb57bf33081d5cfcf6f9ed3d3d7f159c2e2fff579dc341a"
    "07cf33da18bd734c600b96a72bbc4749d5141c90ec8ac328ae52ddfe2e505bdb";
static const char* kK1k = "ffff000000000000000000000000000000000000000000000000000000008000";
static const char* kK1caller =
    "30440220176973c6e09647db98c9d102be12af75097bb06d48d4e6ae88b7f3c072f25ce2"
    "02206e32e794c37dc446f6d5586ba39689f871786a877263114a80e197f6404c221e";
static const char* kK1rfc =
    "30450220749acf843fbbd20be57bd2aca04e20536e3c728fd98c26cd42201d4b2df0057e"
    "0221008059a38dac5c0a67409f7e8e214e4fbbfaaee6cbe084b62d607ba08d2039a06b";

static void expect_row(const uint8_t* sig, const uint32_t* sig_len, int i, const char* want_hex, const char* what) {
  uint8_t want[72];
  const size_t n = hex(want, want_hex);
  CHECK(sig_len[i] == n && memcmp(sig + 72 * i, want, n) == 0, what);
}

int main(int argc, char** argv) {
  const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  JNIEnv envp = &kIface;
  JNIEnv* env = &envp;
  const jlong h = Java_net_corda_core_crypto_gpu_CordaGpu_nativeOpen(env, 0, 0);
  uint8_t d[32], xy[64], want[72];
  hex(d, kR1d);
  struct _jobject bd = {d, 32}, bxy = {xy, 64};
  /* elements: "sample", an empty one, "test" */
  uint8_t msg[10] = {'s', 'a', 'm', 'p', 'l', 'e', 't', 'e', 's', 't'}, sig[3 * 72], status[3], k[3 * 32];
  uint32_t msg_len[3] = {6, 0, 4}, sig_len[3];
  uint64_t msg_off[3] = {0, 10, 6};
  struct _jobject bmsg = {msg, 10}, bmo = {msg_off, 24}, bml = {msg_len, 12}, bsig = {sig, 216}, bsl = {sig_len, 12},
                  bst = {status, 3}, bk = {k, 96};
  if (!gpu) {
    CHECK(h == CG_E_NO_DEVICE, "nativeOpen without a device returns CG_E_NO_DEVICE");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(env, 0, h, 3, 1, &bd) == CG_E_INVALID_ARGUMENT,
          "nativeEcdsaSignerCreate without a context");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerPublicKeys(env, 0, h, CG_E_INVALID_ARGUMENT, &bxy) ==
              CG_E_INVALID_ARGUMENT, "nativeEcdsaSignerPublicKeys with a failed create's handle");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, CG_E_INVALID_ARGUMENT, 3, 0, &bmsg, &bmo, &bml,
                                                                 CG_ECDSA_NONCE_RFC6979, 0, &bsig, 72, &bsl, &bst) ==
              CG_E_INVALID_ARGUMENT, "ecdsaSignBatch with a failed create's handle");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerDestroy(env, 0, h, CG_E_INVALID_ARGUMENT); /* ignored */
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h);
  } else {
    CHECK(h > 0, "nativeOpen");
    struct _jobject bshort = {d, 31};
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(env, 0, h, 3, 1, &bshort) ==
              CG_E_INVALID_ARGUMENT, "a scalar buffer shorter than 32 bytes per key is refused");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(env, 0, h, 4, 1, &bd) == CG_E_INVALID_ARGUMENT,
          "scheme 4 is not an ECDSA scheme");
    /* secp256r1, RFC 6979 mode */
    const jlong s = Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(env, 0, h, 3, 1, &bd);
    CHECK(s > 0, "nativeEcdsaSignerCreate (secp256r1)");
    memset(xy, 0, sizeof xy);
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerPublicKeys(env, 0, h, s, &bxy) == CG_OK,
          "nativeEcdsaSignerPublicKeys");
    hex(want, kR1q);
    CHECK(memcmp(xy, want, 64) == 0, "public key equals RFC 6979 A.2.5's");
    memset(sig, 0xee, sizeof sig);
    memset(status, 9, sizeof status);
    jint rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s, 3, 0, &bmsg, &bmo, &bml,
                                                                     CG_ECDSA_NONCE_RFC6979, 0, &bsig, 72, &bsl, &bst);
    CHECK(rc == CG_OK, "ecdsaSignBatch (RFC 6979 mode)");
    CHECK(status[0] == CG_SIGN_OK && status[1] == CG_SIGN_EMPTY && status[2] == CG_SIGN_OK, "status bytes");
    expect_row(sig, sig_len, 0, kR1sample, "RFC 6979 A.2.5 SHA-256 \"sample\"");
    expect_row(sig, sig_len, 2, kR1test, "RFC 6979 A.2.5 SHA-256 \"test\"");
    memset(want, 0, 72);
    CHECK(sig_len[1] == 0 && memcmp(sig + 72, want, 72) == 0, "an empty element's row and length are zero");
    /* the two signatures verify through nativeVerify with the very buffers signBatch filled */
    uint8_t scheme[3] = {3, 3, 3}, vpk[3 * 64], verdict[3] = {9, 9, 9};
    for (int i = 0; i < 3; ++i) memcpy(vpk + 64 * i, xy, 64);
    struct _jobject bs = {scheme, 3}, bvpk = {vpk, 192}, bv = {verdict, 3};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_nativeVerify(env, 0, h, 3, CG_MODE_DO_VERIFY, &bs, &bvpk, 64, &bsig, 72,
                                                              &bsl, &bmsg, &bmo, &bml, &bv, 0);
    CHECK(rc == CG_OK && verdict[0] == CG_ACCEPT && verdict[1] == CG_ARG_EMPTY && verdict[2] == CG_ACCEPT,
          "the signatures verify on the device");
    /* errors: a key index past the signer, an undersized output buffer, caller mode without nonces */
    uint32_t key_index[3] = {0, 0, 1};
    struct _jobject bidx = {key_index, 12};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s, 3, &bidx, &bmsg, &bmo, &bml,
                                                                CG_ECDSA_NONCE_RFC6979, 0, &bsig, 72, &bsl, &bst);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "key index out of range");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeLastError(env, 0, h);
    CHECK(last_string && strstr(last_string, "element 2"), "the error names the element");
    struct _jobject bsmall = {sig, 215};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s, 3, 0, &bmsg, &bmo, &bml,
                                                                CG_ECDSA_NONCE_RFC6979, 0, &bsmall, 72, &bsl, &bst);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "an output buffer below n * sig_stride bytes is refused");
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s, 3, 0, &bmsg, &bmo, &bml,
                                                                CG_ECDSA_NONCE_CALLER, 0, &bsig, 72, &bsl, &bst);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "caller mode without nonces is refused");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerDestroy(env, 0, h, s);
    /* secp256k1 on the same context: a caller nonce, a nonce of zero, then RFC 6979 mode */
    hex(d, kK1d);
    const jlong s2 = Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerCreate(env, 0, h, 2, 1, &bd);
    CHECK(s2 > 0, "nativeEcdsaSignerCreate (secp256k1)");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerPublicKeys(env, 0, h, s2, &bxy) == CG_OK,
          "nativeEcdsaSignerPublicKeys (secp256k1)");
    hex(want, kK1q);
    CHECK(memcmp(xy, want, 64) == 0, "secp256k1 public key");
    memset(k, 0, sizeof k);
    hex(k, kK1k);  /* element 0: the nonce; element 1 is empty; element 2: k = 0 */
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s2, 3, 0, &bmsg, &bmo, &bml,
                                                                CG_ECDSA_NONCE_CALLER, &bk, &bsig, 72, &bsl, &bst);
    CHECK(rc == CG_OK, "ecdsaSignBatch (caller mode)");
    CHECK(status[0] == CG_SIGN_OK && status[1] == CG_SIGN_EMPTY && status[2] == CG_SIGN_NONCE_INVALID,
          "status bytes (caller mode)");
    expect_row(sig, sig_len, 0, kK1caller, "secp256k1 \"sample\" under the caller's nonce");
    CHECK(sig_len[2] == 0, "a refused nonce leaves no signature");
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_ecdsaSignBatch(env, 0, h, s2, 1, 0, &bmsg, &bmo, &bml,
                                                                CG_ECDSA_NONCE_RFC6979, 0, &bsig, 72, &bsl, 0);
    CHECK(rc == CG_OK, "ecdsaSignBatch with null status");
    expect_row(sig, sig_len, 0, kK1rfc, "secp256k1 \"sample\" under the RFC 6979 nonce");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeEcdsaSignerDestroy(env, 0, h, s2);
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h);
  }
  printf("jni_ecdsa_sign_harness %s: %s\n", gpu ? "gpu" : "cpu", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
