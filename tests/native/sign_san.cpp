// TEST INFRASTRUCTURE ONLY — the host build of the device signing arithmetic
// (cg_sign_host.cpp: the cg_ed25519_sign.h code the HIP kernels compile) as a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer, 8-bit B windows:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all -DCG_ED_BWIN=8 \
//       sign_san.cpp cg_sign_host.cpp
// Reads one case per line from stdin and answers one line each
// (tests/test_sign_host.py compares the answers with the oracle):
//   S <seed hex> <align 0..3> <msg hex>   ->  <public key hex> <signature hex>
//   F <scalar hex, 32 bytes little-endian, < L>  ->  <enc([k]B) hex>
// Every message sits in an exactly-sized heap buffer at the given byte alignment: the
// 4-byte words that hold its bytes and nothing more, so a reader that strays is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
int cgs_bwin(void);
void cgs_fixed_base(const uint32_t* k, uint8_t* enc);
void cgs_sign(const uint8_t* seed, const uint8_t* msg, uint32_t n, uint8_t* pk, uint8_t* sig);
}

static int unhex(const std::string& s, std::vector<uint8_t>& out) {
  if (s == "-") return 0;  // (no bytes)
  if (s.size() % 2) return -1;
  for (size_t i = 0; i < s.size(); i += 2) {
    unsigned v;
    if (sscanf(s.c_str() + i, "%2x", &v) != 1) return -1;
    out.push_back((uint8_t)v);
  }
  return 0;
}

static void puthex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

int main() {
  if (cgs_bwin() != 8) {
    fprintf(stderr, "sign_san: built without -DCG_ED_BWIN=8\n");
    return 2;
  }
  char* line = nullptr;
  size_t cap = 0;
  long cases = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::vector<std::string> f;
    for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) f.push_back(t);
    if (f.empty()) continue;
    if (f[0] == "S" && f.size() == 4) {
      std::vector<uint8_t> seed, msg;
      const int al = atoi(f[2].c_str());
      if (unhex(f[1], seed) || seed.size() != 32 || unhex(f[3], msg) || msg.empty() || al < 0 || al > 3) return 3;
      const size_t words = (al + msg.size() + 3) / 4;
      uint8_t* buf = (uint8_t*)malloc(4 * words);  // 16-byte aligned; exactly the words the bytes touch
      if (!buf) return 4;
      memset(buf, 0xa5, 4 * words);
      memcpy(buf + al, msg.data(), msg.size());
      uint8_t pk[32], sig[64];
      cgs_sign(seed.data(), buf + al, (uint32_t)msg.size(), pk, sig);
      free(buf);
      puthex(pk, 32);
      printf(" ");
      puthex(sig, 64);
      printf("\n");
    } else if (f[0] == "F" && f.size() == 2) {
      std::vector<uint8_t> k;
      if (unhex(f[1], k) || k.size() != 32) return 3;
      uint32_t kw[8];
      memcpy(kw, k.data(), 32);
      uint8_t enc[32];
      cgs_fixed_base(kw, enc);
      puthex(enc, 32);
      printf("\n");
    } else {
      fprintf(stderr, "sign_san: bad line\n");
      return 3;
    }
    ++cases;
  }
  free(line);
  fprintf(stderr, "sign_san: %ld cases\n", cases);
  return 0;
}
