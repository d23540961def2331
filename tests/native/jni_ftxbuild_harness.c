/*
 * Drives the FilteredTransaction-builder natives of integration/jvm/cordagpu_jni.c (compiled
 * against the stub jni.h) through a fake JNIEnv whose direct ByteBuffers are plain C
 * buffers.  `cpu`: no device — nativeFtxBuildLayout (host only) sizes a small batch and
 * refuses undersized buffers and a salt include; buildFilteredBatch refuses a failed
 * context handle and undersized buffers with a status, nothing crashes.  `gpu`: layout,
 * one buildFilteredBatch call, the result through nativeFtxVerify (TRUE / NO_LEAVES), and
 * output buffers one element short (refused, the error carries the needed counts).
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
jint Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxVerify(JNIEnv*, jclass, jlong, jint, jobject, jobject, jobject,
                                                             jobject, jobject, jobject, jobject, jobject, jobject,
                                                             jobject);
jint Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(JNIEnv*, jclass, jint, jobject, jobject, jobject,
                                                                  jobject);
jint Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(JNIEnv*, jclass, jlong, jint, jobject, jobject, jobject,
                                                                jobject, jobject, jobject, jobject, jobject, jobject,
                                                                jobject, jobject, jobject, jobject);

static int failures;
#define CHECK(c, m)                                       \
  do {                                                    \
    if (!(c)) {                                           \
      fprintf(stderr, "FAIL line %d: %s\n", __LINE__, m); \
      ++failures;                                         \
    }                                                     \
  } while (0)

enum { N_TX = 3, N_COMP = 12, MAX_NODES = 32 };

int main(int argc, char** argv) {
  const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  JNIEnv envp = &kIface;
  JNIEnv* env = &envp;
  const jlong h = Java_net_corda_core_crypto_gpu_CordaGpu_nativeOpen(env, 0, 0);
  /* tx 0: 6 components, inputs 0, 1 and the time window (4) visible; tx 1: salt only;
   * tx 2: 5 components, nothing visible */
  uint32_t comp_start[N_TX + 1] = {0, 6, 7, 12};
  uint8_t include[N_COMP] = {1, 1, 0, 0, 1, 0, /**/ 0, /**/ 0, 0, 0, 0, 0};
  uint32_t comp_len[N_COMP];
  uint64_t comp_off[N_COMP];
  uint8_t arena[N_COMP * 40], salts[32 * N_TX];
  for (int c = 0; c < N_COMP; ++c) {
    comp_len[c] = 17 + 2 * (uint32_t)c;
    comp_off[c] = 40 * (uint64_t)c;
  }
  for (size_t i = 0; i < sizeof arena; ++i) arena[i] = (uint8_t)(i * 131 + 7);
  for (size_t i = 0; i < sizeof salts; ++i) salts[i] = (uint8_t)(i * 29 + 3);
  uint32_t fstart[N_TX + 1], nstart[N_TX + 1], findex[N_COMP];
  uint8_t nonces[32 * N_COMP], kind[MAX_NODES], nhash[32 * MAX_NODES], roots[32 * N_TX];
  struct _jobject bcs = {comp_start, sizeof comp_start}, binc = {include, sizeof include},
                  bfs = {fstart, sizeof fstart}, bns = {nstart, sizeof nstart}, barena = {arena, sizeof arena},
                  boff = {comp_off, sizeof comp_off}, blen = {comp_len, sizeof comp_len}, bsalts = {salts, sizeof salts},
                  broots = {roots, sizeof roots};
  jint rc = Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(env, 0, N_TX, &bcs, &binc, &bfs, &bns);
  CHECK(rc == CG_OK, "nativeFtxBuildLayout");
  CHECK(fstart[1] == 3 && fstart[2] == 3 && fstart[3] == 3, "filtered component counts");
  /* tx 0 (8 padded leaves; 0, 1 and 4 included): I I N  L  N | I L N  L  N | N = 11 nodes; then one each */
  CHECK(nstart[1] == 11 && nstart[2] == 12 && nstart[3] == 13, "node counts");
  const uint32_t n_f = fstart[N_TX], n_n = nstart[N_TX];
  struct _jobject short_cs = {comp_start, sizeof comp_start - 1}, short_inc = {include, sizeof include - 1};
  CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(env, 0, N_TX, &short_cs, &binc, &bfs, &bns) ==
            CG_E_INVALID_ARGUMENT, "a comp_start buffer below n_tx + 1 entries is refused");
  CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(env, 0, N_TX, &bcs, &short_inc, &bfs, &bns) ==
            CG_E_INVALID_ARGUMENT, "an include buffer below one byte per component is refused");
  CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(env, 0, -1, &bcs, &binc, &bfs, &bns) ==
            CG_E_INVALID_ARGUMENT, "a negative count is refused");
  include[5] = 1; /* the salt of tx 0 */
  CHECK(Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxBuildLayout(env, 0, N_TX, &bcs, &binc, &bfs, &bns) ==
            CG_E_INVALID_ARGUMENT, "a salt include is refused");
  include[5] = 0;
  struct _jobject bfi = {findex, 4 * n_f}, bnon = {nonces, 32 * n_f}, bkind = {kind, n_n}, bnh = {nhash, 32 * n_n};
  if (!gpu) {
    CHECK(h == CG_E_NO_DEVICE || h > 0, "nativeOpen returns a handle or CG_E_NO_DEVICE");
    if (h > 0) Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h); /* (run on a box with a device) */
    const jlong none = CG_E_NO_DEVICE;
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(env, 0, none, N_TX, &barena, &boff, &blen, &bcs, &bsalts,
                                                                    &binc, &bfs, &bfi, &bnon, &bns, &bkind, &bnh, &broots);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "buildFilteredBatch with a failed open's handle");
    struct _jobject short_roots = {roots, sizeof roots - 1};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(env, 0, none, N_TX, &barena, &boff, &blen, &bcs,
                                                                    &bsalts, &binc, &bfs, &bfi, &bnon, &bns, &bkind, &bnh,
                                                                    &short_roots);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "a roots buffer below 32 bytes per tx is refused");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, none); /* ignored */
  } else {
    CHECK(h > 0, "nativeOpen");
    uint32_t f2[N_TX + 1], n2[N_TX + 1];
    struct _jobject bf2 = {f2, sizeof f2}, bn2 = {n2, sizeof n2};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(env, 0, h, N_TX, &barena, &boff, &blen, &bcs, &bsalts,
                                                                    &binc, &bf2, &bfi, &bnon, &bn2, &bkind, &bnh, &broots);
    CHECK(rc == CG_OK, "buildFilteredBatch");
    CHECK(memcmp(f2, fstart, sizeof f2) == 0 && memcmp(n2, nstart, sizeof n2) == 0, "the call's own layout");
    CHECK(findex[0] == 0 && findex[1] == 1 && findex[2] == 4, "filtered component indices");
    static const uint8_t want_kind[13] = {0, 0, 2, 1, 2, 0, 1, 2, 1, 2, 2, 1, 1};
    CHECK(memcmp(kind, want_kind, 13) == 0, "node kinds");
    CHECK(memcmp(nhash + 32 * 11, roots + 32, 32) == 0 && memcmp(nhash + 32 * 12, roots + 64, 32) == 0,
          "a transaction with nothing visible is the single node Leaf(root)");
    uint64_t foff[N_COMP];
    uint32_t flen[N_COMP];
    for (uint32_t j = 0; j < n_f; ++j) {
      foff[j] = comp_off[findex[j]];
      flen[j] = comp_len[findex[j]];
    }
    uint8_t res[N_TX] = {9, 9, 9};
    struct _jobject bfo = {foff, 8 * n_f}, bfl = {flen, 4 * n_f}, bres = {res, sizeof res};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_nativeFtxVerify(env, 0, h, N_TX, &barena, &bfo, &bfl, &bfs, &bnon, &bns,
                                                                 &bkind, &bnh, &broots, &bres);
    CHECK(rc == CG_OK && res[0] == CG_FTX_TRUE && res[1] == CG_FTX_NO_LEAVES && res[2] == CG_FTX_NO_LEAVES,
          "the built transactions verify on the device");
    /* output buffers one element short */
    struct _jobject bkind_short = {kind, n_n - 1}, bnon_short = {nonces, 32 * n_f - 1};
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(env, 0, h, N_TX, &barena, &boff, &blen, &bcs, &bsalts,
                                                                    &binc, &bf2, &bfi, &bnon, &bn2, &bkind_short, &bnh,
                                                                    &broots);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "a node_kind buffer one short is refused");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeLastError(env, 0, h);
    CHECK(last_string && strstr(last_string, "3 filtered components") && strstr(last_string, "13 nodes"),
          "the error carries the needed counts");
    rc = Java_net_corda_core_crypto_gpu_CordaGpu_buildFilteredBatch(env, 0, h, N_TX, &barena, &boff, &blen, &bcs, &bsalts,
                                                                    &binc, &bf2, &bfi, &bnon_short, &bn2, &bkind, &bnh,
                                                                    &broots);
    CHECK(rc == CG_E_INVALID_ARGUMENT, "a nonces buffer one byte short is refused");
    Java_net_corda_core_crypto_gpu_CordaGpu_nativeClose(env, 0, h);
  }
  printf("jni_ftxbuild_harness %s: %s\n", gpu ? "gpu" : "cpu", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
