// TEST INFRASTRUCTURE ONLY — the host build of the FilteredTransaction builder's device
// logic (cg_ftxbuild_host.cpp: cg_pmt_build.h, cg_ftx_layout.h, cg_sha256.h) as a
// stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all ftxbuild_san.cpp cg_ftxbuild_host.cpp
// Reads one transaction per line from stdin,
//   <salt hex> <include mask, one 0/1 per component> <component hex>,<component hex>,...
// ("-" for a transaction without components); an empty line (or the end of the input) runs
// the batch read so far through cgf_layout and cgf_build and prints its seven output arrays,
// one "name hex" line each (32-bit arrays little-endian), then "end".
// tests/test_ftx_build_host.py compares them with the oracle.  Every input and output
// array sits in an exactly-sized heap buffer, so a reader or writer that strays is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
int cgf_layout(size_t n_tx, const uint32_t* comp_start, const uint8_t* include, uint32_t* fcomp_start_out,
               uint32_t* node_start_out);
int cgf_build(size_t n_tx, const uint8_t* arena, const uint64_t* comp_off, const uint32_t* comp_len,
              const uint32_t* comp_start, const uint8_t* salts, const uint8_t* include, uint32_t* fcomp_start_out,
              uint32_t* fcomp_index_out, uint8_t* nonces_out, uint32_t* node_start_out, uint8_t* node_kind_out,
              uint8_t* node_hash_out, uint8_t* root_out);
}

static int unhex(const char* s, size_t n, std::vector<uint8_t>& out) {
  if (n % 2) return -1;
  for (size_t i = 0; i < n; i += 2) {
    unsigned v;
    if (sscanf(s + i, "%2x", &v) != 1) return -1;
    out.push_back((uint8_t)v);
  }
  return 0;
}

static void hexline(const char* name, const void* p, size_t n) {
  printf("%s ", name);
  for (size_t i = 0; i < n; ++i) printf("%02x", ((const uint8_t*)p)[i]);
  printf("\n");
}

// exactly-sized heap copy (malloc(0) stays a valid, unreadable pointer)
template <class T>
static T* exact(const std::vector<T>& v) {
  T* p = (T*)malloc(v.size() * sizeof(T));
  if (v.size()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

struct BatchIn {
  std::vector<uint8_t> arena, salts, include;
  std::vector<uint64_t> comp_off;
  std::vector<uint32_t> comp_len, comp_start{0};
};

static int run(const BatchIn& b) {
  const size_t n_tx = b.comp_start.size() - 1;
  uint8_t *arena = exact(b.arena), *salts = exact(b.salts), *include = exact(b.include);
  uint64_t* comp_off = exact(b.comp_off);
  uint32_t *comp_len = exact(b.comp_len), *comp_start = exact(b.comp_start);
  uint32_t* fs = (uint32_t*)malloc(4 * (n_tx + 1));
  uint32_t* ns = (uint32_t*)malloc(4 * (n_tx + 1));
  if (cgf_layout(n_tx, comp_start, include, fs, ns) != 0) return 5;
  const size_t n_f = fs[n_tx], n_n = ns[n_tx];
  uint32_t* fi = (uint32_t*)malloc(4 * n_f);
  uint8_t* nonces = (uint8_t*)malloc(32 * n_f);
  uint8_t* kind = (uint8_t*)malloc(n_n);
  uint8_t* nhash = (uint8_t*)malloc(32 * n_n);
  uint8_t* roots = (uint8_t*)malloc(32 * n_tx);
  uint32_t* fs2 = (uint32_t*)malloc(4 * (n_tx + 1));
  uint32_t* ns2 = (uint32_t*)malloc(4 * (n_tx + 1));
  const int rc = cgf_build(n_tx, arena, comp_off, comp_len, comp_start, salts, include, fs2, fi, nonces, ns2, kind, nhash,
                           roots);
  if (rc != 0 || memcmp(fs, fs2, 4 * (n_tx + 1)) || memcmp(ns, ns2, 4 * (n_tx + 1))) return 6;
  hexline("fcomp_start", fs, 4 * (n_tx + 1));
  hexline("fcomp_index", fi, 4 * n_f);
  hexline("nonces", nonces, 32 * n_f);
  hexline("node_start", ns, 4 * (n_tx + 1));
  hexline("node_kind", kind, n_n);
  hexline("node_hash", nhash, 32 * n_n);
  hexline("roots", roots, 32 * n_tx);
  printf("end\n");
  for (void* p : {(void*)arena, (void*)salts, (void*)include, (void*)comp_off, (void*)comp_len, (void*)comp_start,
                  (void*)fs, (void*)ns, (void*)fi, (void*)nonces, (void*)kind, (void*)nhash, (void*)roots, (void*)fs2,
                  (void*)ns2})
    free(p);
  return 0;
}

int main() {
  char* line = nullptr;
  size_t cap = 0;
  long batches = 0;
  BatchIn b;
  ssize_t got;
  while ((got = getline(&line, &cap, stdin)) > 0) {
    std::vector<std::string> f;
    for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) f.push_back(t);
    if (f.empty()) {
      if (const int rc = run(b)) return rc;
      ++batches;
      b = BatchIn();
      continue;
    }
    if (f.size() != 3 || unhex(f[0].c_str(), f[0].size(), b.salts) || b.salts.size() % 32) return 3;
    size_t k = 0;
    if (f[2] != "-") {
      size_t at = 0;
      for (;;) {
        const size_t comma = f[2].find(',', at);
        const size_t len = (comma == std::string::npos ? f[2].size() : comma) - at;
        const size_t before = b.arena.size();
        if (unhex(f[2].c_str() + at, len, b.arena)) return 3;
        b.comp_off.push_back(before);
        b.comp_len.push_back((uint32_t)(b.arena.size() - before));
        ++k;
        if (comma == std::string::npos) break;
        at = comma + 1;
      }
    }
    if ((f[1] == "-" ? 0 : f[1].size()) != k) return 3;
    for (size_t i = 0; i < k; ++i) b.include.push_back(f[1][i] == '1');
    b.comp_start.push_back(b.comp_start.back() + (uint32_t)k);
  }
  if (b.comp_start.size() > 1) {
    if (const int rc = run(b)) return rc;
    ++batches;
  }
  free(line);
  fprintf(stderr, "ftxbuild_san: %ld batches\n", batches);
  return 0;
}
