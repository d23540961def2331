// TEST INFRASTRUCTURE ONLY — the host build of the device ECDSA signing arithmetic
// (cg_ecdsa_sign_host.cpp: the cg_ecdsa_sign.h code the HIP kernels compile) as a stand-alone
// program for AddressSanitizer + UndefinedBehaviorSanitizer, 8-bit windows:
//   g++ -fsanitize=address,undefined -fno-sanitize-recover=all -DCG_ECDSA_SIGN_WIN=8 \
//       ecdsa_sign_san.cpp cg_ecdsa_sign_host.cpp
// argv[1]: a file of cases with their expectations (tests/test_ecdsa_sign_host.py writes it
// from the oracle), one per line; exits 0 when every case gives its expectation:
//   S <scheme> <nonce mode> <d hex> <k hex | -> <align 0..3> <msg hex | -> <status> <sig hex | ->
//   P <scheme> <d hex> <X || Y hex>
//   R <order hex> <d hex> <digest hex> <k hex>
// Every message sits in an exactly-sized heap buffer at the given byte alignment: the
// 4-byte words that hold its bytes and nothing more, so a reader that strays is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

extern "C" {
int cges_win(void);
uint32_t cges_sign(int scheme, const uint8_t* d_be, const uint8_t* msg, uint32_t n, int mode, const uint8_t* k_be,
                   uint8_t* sig, uint32_t* sig_len);
int cges_pubkey(int scheme, const uint8_t* d_be, uint8_t* xy);
uint32_t cges_rfc6979(const uint8_t* order_be, const uint8_t* d_be, const uint8_t* h1, uint8_t* k_be);
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

int main(int argc, char** argv) {
  if (cges_win() != 8) {
    fprintf(stderr, "ecdsa_sign_san: built without -DCG_ECDSA_SIGN_WIN=8\n");
    return 2;
  }
  FILE* in = argc > 1 ? fopen(argv[1], "r") : nullptr;
  if (!in) {
    fprintf(stderr, "ecdsa_sign_san: no case file\n");
    return 2;
  }
  char* line = nullptr;
  size_t cap = 0;
  long cases = 0, bad = 0;
  while (getline(&line, &cap, in) > 0) {
    std::vector<std::string> f;
    for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n")) f.push_back(t);
    if (f.empty()) continue;
    ++cases;
    bool ok = false;
    if (f[0] == "S" && f.size() == 9) {
      std::vector<uint8_t> d, k, msg, want;
      const int scheme = atoi(f[1].c_str()), mode = atoi(f[2].c_str()), al = atoi(f[5].c_str());
      if (unhex(f[3], d) || d.size() != 32 || unhex(f[4], k) || (!k.empty() && k.size() != 32) || unhex(f[6], msg) ||
          unhex(f[8], want) || al < 0 || al > 3)
        return 3;
      const size_t words = (al + msg.size() + 3) / 4;
      uint8_t* buf = (uint8_t*)malloc(words ? 4 * words : 1);  // 16-byte aligned; exactly the words the bytes touch
      if (!buf) return 4;
      memset(buf, 0xa5, 4 * words);
      if (!msg.empty()) memcpy(buf + al, msg.data(), msg.size());
      uint8_t sig[72];
      uint32_t len = 0;
      // (an empty message is never read: it gets no buffer at all)
      const uint32_t st = cges_sign(scheme, d.data(), msg.empty() ? nullptr : buf + al, (uint32_t)msg.size(), mode,
                                    k.empty() ? nullptr : k.data(), sig, &len);
      free(buf);
      ok = st == (uint32_t)atoi(f[7].c_str()) && len == want.size() && (len == 0 || memcmp(sig, want.data(), len) == 0);
      for (uint32_t i = len; ok && i < 72; ++i) ok = sig[i] == 0;
    } else if (f[0] == "P" && f.size() == 4) {
      std::vector<uint8_t> d, want;
      if (unhex(f[2], d) || d.size() != 32 || unhex(f[3], want) || want.size() != 64) return 3;
      uint8_t xy[64];
      ok = cges_pubkey(atoi(f[1].c_str()), d.data(), xy) == 0 && memcmp(xy, want.data(), 64) == 0;
    } else if (f[0] == "R" && f.size() == 5) {
      std::vector<uint8_t> order, d, h1, want;
      if (unhex(f[1], order) || order.size() != 32 || unhex(f[2], d) || d.size() != 32 || unhex(f[3], h1) ||
          h1.size() != 32 || unhex(f[4], want) || want.size() != 32)
        return 3;
      uint8_t k[32];
      cges_rfc6979(order.data(), d.data(), h1.data(), k);
      ok = memcmp(k, want.data(), 32) == 0;
    } else {
      fprintf(stderr, "ecdsa_sign_san: bad line %ld\n", cases);
      return 3;
    }
    if (!ok) {
      fprintf(stderr, "ecdsa_sign_san: case %ld (%s) differs from its expectation\n", cases, f[0].c_str());
      ++bad;
    }
  }
  free(line);
  fclose(in);
  fprintf(stderr, "ecdsa_sign_san: %ld cases, %ld wrong\n", cases, bad);
  return bad ? 1 : 0;
}
