/*
 * A plain C99 caller of the FilteredTransaction builder through include/cordagpu.h.
 * `cpu`: no device — cg_ftx_build_layout (a pure host function) on a small batch, its
 * argument errors, and cg_ftx_build_batch refusing a null context.  `gpu`: one
 * cg_ftx_build_layout + cg_ftx_build_batch call, the result handed to cg_ftx_verify_batch
 * and compared with cg_txid_batch's ids; inputs and outputs are printed as "name value"
 * lines, which tests/test_gpu_ftx_build.py compares with the oracle.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cordagpu.h"

static int failures;
#define CHECK(c, m)                                       \
  do {                                                    \
    if (!(c)) {                                           \
      fprintf(stderr, "FAIL line %d: %s\n", __LINE__, m); \
      ++failures;                                         \
    }                                                     \
  } while (0)

enum { N_TX = 4, N_COMP = 17 };
/* 5 + 1 + 8 + 3 components; the last of each transaction is the serialized salt */
static const uint32_t kCompStart[N_TX + 1] = {0, 5, 6, 14, 17};
static const uint8_t kInclude[N_COMP] = {1, 0, 0, 1, 0, /**/ 0, /**/ 0, 0, 0, 0, 0, 1, 0, 0, /**/ 0, 0, 0};
static const uint32_t kCompLen[N_COMP] = {50, 61, 300, 40, 44, 44, 48, 48, 55, 56, 23, 24, 150, 44, 1, 88, 44};

static void hexline(const char* name, const uint8_t* p, size_t n) {
  printf("%s ", name);
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
}

static void intline(const char* name, const uint32_t* p, size_t n) {
  printf("%s", name);
  for (size_t i = 0; i < n; ++i) printf(" %u", (unsigned)p[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  uint64_t comp_off[N_COMP];
  size_t arena_bytes = 0;
  for (int c = 0; c < N_COMP; ++c) {
    comp_off[c] = arena_bytes;
    arena_bytes += kCompLen[c];
  }
  uint8_t* arena = (uint8_t*)malloc(arena_bytes);
  uint8_t salts[32 * N_TX];
  uint32_t x = 2463534242u; /* xorshift32 */
  for (size_t i = 0; i < arena_bytes + sizeof salts; ++i) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    if (i < arena_bytes)
      arena[i] = (uint8_t)(x >> 8);
    else
      salts[i - arena_bytes] = (uint8_t)(x >> 8);
  }
  uint32_t fstart[N_TX + 1], nstart[N_TX + 1];
  CHECK(cg_ftx_build_layout(N_TX, kCompStart, kInclude, fstart, nstart) == CG_OK, "layout");
  CHECK(fstart[N_TX] == 3 && fstart[1] == 2 && fstart[2] == 2 && fstart[3] == 3, "filtered component counts");
  /* tx 1 (salt only) and tx 3 (empty mask) are the single node Leaf(root) */
  CHECK(nstart[2] - nstart[1] == 1 && nstart[4] - nstart[3] == 1, "single-node trees");
  uint32_t f2[N_TX + 1], n2[N_TX + 1];
  CHECK(cg_ftx_build_layout(N_TX, 0, kInclude, f2, n2) == CG_E_INVALID_ARGUMENT, "layout: null comp_start");
  CHECK(cg_ftx_build_layout(N_TX, kCompStart, 0, f2, n2) == CG_E_INVALID_ARGUMENT, "layout: null include");
  CHECK(cg_ftx_build_layout(N_TX, kCompStart, kInclude, 0, n2) == CG_E_INVALID_ARGUMENT, "layout: null output");
  uint8_t bad[N_COMP];
  memcpy(bad, kInclude, N_COMP);
  bad[13] = 1; /* the salt of tx 2 */
  CHECK(cg_ftx_build_layout(N_TX, kCompStart, bad, f2, n2) == CG_E_INVALID_ARGUMENT, "layout: salt included");
  const uint32_t down[N_TX + 1] = {0, 5, 4, 14, 17};
  CHECK(cg_ftx_build_layout(N_TX, down, kInclude, f2, n2) == CG_E_INVALID_ARGUMENT, "layout: decreasing comp_start");
  CHECK(cg_ftx_build_layout(0, kCompStart, kInclude, f2, n2) == CG_OK && f2[0] == 0 && n2[0] == 0, "layout: no tx");

  const size_t n_f = fstart[N_TX], n_n = nstart[N_TX];
  uint32_t* findex = (uint32_t*)calloc(n_f, 4);
  uint8_t* nonces = (uint8_t*)calloc(n_f, 32);
  uint8_t* kind = (uint8_t*)calloc(n_n, 1);
  uint8_t* nhash = (uint8_t*)calloc(n_n, 32);
  uint8_t roots[32 * N_TX], ids[32 * N_TX];
  if (!gpu) {
    CHECK(cg_ftx_build_batch(0, N_TX, arena, arena_bytes, comp_off, kCompLen, kCompStart, salts, kInclude, n_f, n_n, f2,
                             findex, nonces, n2, kind, nhash, roots) == CG_E_INVALID_ARGUMENT,
          "build without a context");
  } else {
    cg_ctx* ctx = 0;
    CHECK(cg_open(0, &ctx) == CG_OK, "cg_open");
    if (!ctx) return 1;
    cg_status st = cg_ftx_build_batch(ctx, N_TX, arena, arena_bytes, comp_off, kCompLen, kCompStart, salts, kInclude,
                                      n_f, n_n, f2, findex, nonces, n2, kind, nhash, roots);
    CHECK(st == CG_OK, cg_last_error(ctx));
    CHECK(memcmp(f2, fstart, sizeof fstart) == 0 && memcmp(n2, nstart, sizeof nstart) == 0, "the call's own layout");
    CHECK(cg_txid_batch(ctx, N_TX, arena, arena_bytes, comp_off, kCompLen, kCompStart, salts, ids) == CG_OK, "txid");
    CHECK(memcmp(ids, roots, sizeof ids) == 0, "roots equal the transaction ids");
    /* round trip: the filtered components are the same arena gathered with fcomp_index */
    uint64_t foff[N_COMP];
    uint32_t flen[N_COMP];
    for (size_t j = 0; j < n_f; ++j) {
      foff[j] = comp_off[findex[j]];
      flen[j] = kCompLen[findex[j]];
    }
    uint8_t res[N_TX];
    st = cg_ftx_verify_batch(ctx, N_TX, arena, arena_bytes, foff, flen, fstart, nonces, nstart, kind, nhash, roots, res);
    CHECK(st == CG_OK, cg_last_error(ctx));
    CHECK(res[0] == CG_FTX_TRUE && res[1] == CG_FTX_NO_LEAVES && res[2] == CG_FTX_TRUE && res[3] == CG_FTX_NO_LEAVES,
          "verify() of the built transactions");
    /* a capacity one short: refused, the message carries the needed counts */
    st = cg_ftx_build_batch(ctx, N_TX, arena, arena_bytes, comp_off, kCompLen, kCompStart, salts, kInclude, n_f,
                            n_n - 1, f2, findex, nonces, n2, kind, nhash, roots);
    char want[32];
    snprintf(want, sizeof want, "%u nodes", (unsigned)n_n);
    CHECK(st == CG_E_INVALID_ARGUMENT && strstr(cg_last_error(ctx), want), "node capacity one short");
    cg_close(ctx);
    uint32_t counts[N_TX];
    for (int t = 0; t < N_TX; ++t) counts[t] = kCompStart[t + 1] - kCompStart[t];
    intline("counts", counts, N_TX);
    intline("comp_len", kCompLen, N_COMP);
    hexline("arena", arena, arena_bytes);
    hexline("salts", salts, sizeof salts);
    hexline("include", kInclude, N_COMP);
    intline("fcomp_start", fstart, N_TX + 1);
    intline("fcomp_index", findex, n_f);
    intline("node_start", nstart, N_TX + 1);
    hexline("node_kind", kind, n_n);
    hexline("node_hash", nhash, 32 * n_n);
    hexline("nonces", nonces, 32 * n_f);
    hexline("roots", roots, sizeof roots);
  }
  free(findex);
  free(nonces);
  free(kind);
  free(nhash);
  free(arena);
  printf("ftx_build_abi %s: %s\n", gpu ? "gpu" : "cpu", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
