/*
 * Drives the signing natives of integration/jvm/cordagpu_jni.c (compiled against the stub
 * jni.h) through a fake JNIEnv whose direct ByteBuffers are plain C buffers.  `cpu`: no
 * device — every native refuses a failed context or signer handle with a status, nothing
 * crashes; `gpu`: RFC 8032 tests 1-3 as three keys of one signer, signed in one signBatch
 * call with a non-monotone key index and an empty element, public keys and signatures
 * compared byte for byte with the RFC's, then verified through nativeVerify.
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
jlong Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerCreate(JNIEnv*, jclass, jlong, jint, jobject);
jint Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerPublicKeys(JNIEnv*, jclass, jlong, jlong, jobject);
void Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerDestroy(JNIEnv*, jclass, jlong, jlong);
jint Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(JNIEnv*, jclass, jlong, jlong, jint, jobject, jobject, jobject,
                                                       jobject, jobject, jobject);

static int failures;
#define CHECK(c, m)                                       \
  do {                                                    \
    if (!(c)) {                                           \
      fprintf(stderr, "FAIL line %d: %s\n", __LINE__, m); \
      ++failures;                                         \
    }                                                     \
  } while (0)

static void hex(uint8_t* out, const char* h) {
  for (size_t i = 0; h[2 * i]; ++i) {
    unsigned v;
    sscanf(h + 2 * i, "%2x", &v);
    out[i] = (uint8_t)v;
  }
}

/* RFC 8032 section 7.1, tests 1-3: seed, public key, message, signature */
static const char* kSeed[3] = {"9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
                               "4ccd089b28ff96da9db6c346ec114e0f5b8a319f35aba624da8cf6ed4fb8a6fb",
                               "c5aa8df43f9f837bedb7442f31dcb7b166d38535076f094b85ce3a2e0b4458f7"};
static const char* kPk[3] = {"d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
                             "3d4017c3e843895a92b70aa74d1b7ebc9c982ccf2ec4968cc0cd55f12af4660c",
                             "fc51cd8e6218a1a38da47ed00230f0580816ed13ba3303ac5deb911548908025"};
static const char* kSig[3] = {
    "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46b"
    "d25bf5f0595bbe24655141438e7a100b",
    "92a009a9f0d4cab8720e820b5f642540a2b27b5416503f8fb3762223ebdb69da085ac1e43e15996e458f3613d0f11d8c"
    "387b2eaeb4302aeeb00d291612bb0c00",
    "6291d657deec24024827e69c3abe01a30ce548a284743a445e3680d7db5ac3ac18ff9b538d16f290ae67f760984dc659"
    "4a7c15e9716ed28dc027beceea1ec40a"};

int main(int argc, char** argv) {
  const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  JNIEnv envp = &kIface;
  JNIEnv* env = &envp;
  const jlong h = Java_net_corda_core_crypto_gpu_CordaGpu_nativeOpen(env, 0, 0);
  uint8_t seeds[96], pk[96];
  for (int j = 0; j < 3; ++j) hex(seeds + 32 * j, kSeed[j]);
  struct _jobject bseeds = {seeds, 96}, bpk = {pk, 96};
  /* elements: test 3 (2 bytes), an empty one, test 2 (1 byte), test 2 again; test 1 signs the
   * empty message, which doSign refuses, so its key is only checked through its public key */
  uint8_t msg[3] = {0xaf, 0x82, 0x72}, sig[4 * 64], status[4];
  uint32_t key_index[4] = {2, 0, 1, 1}, msg_len[4] = {2, 0, 1, 1};
  uint64_t msg_off[4] = {0, 3, 2, 2};
  struct _jobject bidx = {key_index, 16}, bmsg = {msg, 3}, bmo = {msg_off, 32}, bml = {msg_len, 16}, bsig = {sig, 256},
                  bst = {status, 4};
  if (!gpu) {
    CHECK(h == CG_E_NO_DEVICE, "nativeOpen without a device returns CG_E_NO_DEVICE");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerCreate(env, 0, h, 3, &bseeds) == CG_E_INVALID_ARGUMENT,
          "nativeSignerCreate without a context");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerPublicKeys(env, 0, h, CG_E_INVALID_ARGUMENT, &bpk) ==
              CG_E_INVALID_ARGUMENT, "nativeSignerPublicKeys with a failed create's handle");
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(env, 0, h, CG_E_INVALID_ARGUMENT, 4, &bidx, &bmsg, &bmo,
                                                            &bml, &bsig, &bst) == CG_E_INVALID_ARGUMENT,
          "signBatch with a failed create's handle");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerDestroy(env, 0, h, CG_E_INVALID_ARGUMENT); /* ignored */
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h);
  } else {
    CHECK(h > 0, "nativeOpen");
    struct _jobject bshort = {seeds, 64};
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerCreate(env, 0, h, 3, &bshort) == CG_E_INVALID_ARGUMENT,
          "a seed buffer shorter than 32 bytes per key is refused");
    const jlong s = Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerCreate(env, 0, h, 3, &bseeds);
    CHECK(s > 0, "nativeSignerCreate");
    memset(pk, 0, sizeof pk);
    CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerPublicKeys(env, 0, h, s, &bpk) == CG_OK,
          "nativeSignerPublicKeys");
    uint8_t want[64];
    for (int j = 0; j < 3; ++j) {
      hex(want, kPk[j]);
      CHECK(memcmp(pk + 32 * j, want, 32) == 0, "public key equals RFC 8032's");
    }
    memset(sig, 0xee, sizeof sig);
    memset(status, 9, sizeof status);
    jint rc = Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(env, 0, h, s, 4, &bidx, &bmsg, &bmo, &bml, &bsig, &bst);
    CHECK(rc == CG_OK, "signBatch");
    CHECK(status[0] == CG_SIGN_OK && status[1] == CG_SIGN_EMPTY && status[2] == CG_SIGN_OK && status[3] == CG_SIGN_OK,
          "status bytes");
    hex(want, kSig[2]);
    CHECK(memcmp(sig, want, 64) == 0, "RFC 8032 test 3 signature");
    hex(want, kSig[1]);
    CHECK(memcmp(sig + 128, want, 64) == 0 && memcmp(sig + 192, want, 64) == 0, "RFC 8032 test 2 signature, twice");
    memset(want, 0, 64);
    CHECK(memcmp(sig + 64, want, 64) == 0, "an empty element's signature row is zero");
    /* null key index: every element under key 0; null status */
    uint32_t one_len[1] = {2};
    uint64_t one_off[1] = {0};
    struct _jobject b1o = {one_off, 8}, b1l = {one_len, 4}, b1s = {sig, 64};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(env, 0, h, s, 1, 0, &bmsg, &b1o, &b1l, &b1s, 0);
    CHECK(rc == CG_OK, "signBatch with null key index and null status");
    /* ...which verifies under key 0 through nativeVerify */
    uint8_t scheme[1] = {4}, vpk[64] = {0}, verdict[1] = {9};
    uint32_t sig_len[1] = {64};
    memcpy(vpk, pk, 32);
    struct _jobject bs = {scheme, 1}, bvpk = {vpk, 64}, bsl = {sig_len, 4}, bv = {verdict, 1};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_nativeVerify(env, 0, h, 1, CG_MODE_DO_VERIFY, &bs, &bvpk, 64, &b1s, 64,
                                                              &bsl, &bmsg, &b1o, &b1l, &bv, 0);
    CHECK(rc == CG_OK && verdict[0] == CG_ACCEPT, "the signature verifies on the device");
    /* errors: a key index past the signer, an undersized output buffer */
    key_index[3] = 3;
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(env, 0, h, s, 4, &bidx, &bmsg, &bmo, &bml, &bsig, &bst);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "key index out of range");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeLastError(env, 0, h);
    CHECK(last_string && strstr(last_string, "element 3"), "the error names the element");
    key_index[3] = 1;
    struct _jobject bsmall = {sig, 255};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_signBatch(env, 0, h, s, 4, &bidx, &bmsg, &bmo, &bml, &bsmall, &bst);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "an output buffer below n * 64 bytes is refused");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeSignerDestroy(env, 0, h, s);
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h);
  }
  printf("jni_sign_harness %s: %s\n", gpu ? "gpu" : "cpu", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
