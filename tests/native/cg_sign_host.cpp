// Host build of the device Ed25519 signing arithmetic (cg_ed25519_sign.h: the exact code
// the HIP kernels compile), used only by tests/test_sign_host.py and
// tests/native/sign_san.cpp to check it against the oracle without a GPU.  Built twice:
// with the default 16-bit B windows (libcg_sign_host.so) and with -DCG_ED_BWIN=8
// (libcg_sign_host_w8.so, the sanitizer build's window size).  Not part of the product.
#include <stdint.h>
#include <string.h>

#include "cg_ed25519_sign.h"

using namespace cg;

namespace {

// the device's shared tables j * 2^(32 s) B, each entry built on first use with the
// device's own code (a scalar touches 16 or 32 of them)
ge_precomp g_btab_store[kBTables][kBTabEntries];
uint8_t g_btab_built[kBTables][kBTabEntries];

void get_b(uint32_t s, uint32_t j, ge_precomp& p) {
  if (!g_btab_built[s][j]) {
    ed25519_btab_entry(g_btab_store[s][j], s, j);
    g_btab_built[s][j] = 1;
  }
  p = g_btab_store[s][j];
}

}  // namespace

extern "C" {

int cgs_bwin(void) { return kBWin; }

// seed (32 bytes) -> a mod L (8 words), prefix (8 words), A = enc([a]B) (32 bytes)
void cgs_expand_seed(const uint8_t* seed, uint32_t* a, uint32_t* prefix, uint8_t* pk) {
  uint32_t sw[8], ab[8];
  memcpy(sw, seed, 32);
  ed25519_expand_seed(a, prefix, sw);
  ed25519_public_key(ab, a, get_b);
  memcpy(pk, ab, 32);
}

// enc([k]B) for k < L (8 little-endian words)
void cgs_fixed_base(const uint32_t* k, uint8_t* enc) {
  uint32_t e[8];
  ed25519_fixed_base_enc(e, k, get_b);
  memcpy(enc, e, 32);
}

// (a b + c) mod L
void cgs_sc_muladd(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
  sc_muladd_mod(out, a, b, c);
}

void cgs_sc_reduce256(const uint32_t* x, uint32_t* out) { sc_reduce256(out, x); }

// SHA-512(prefix || msg[0..n)) with a prefix of pw = 0, 8 or 16 words; returns -1 for another pw
int cgs_sha512_prefixed(int pw, const uint32_t* prefix, const uint8_t* msg, uint32_t n, uint8_t* out) {
  uint32_t d[16];
  if (pw == 0)
    sha512_prefixed<0>(d, prefix, msg, n);
  else if (pw == 8)
    sha512_prefixed<8>(d, prefix, msg, n);
  else if (pw == 16)
    sha512_prefixed<16>(d, prefix, msg, n);
  else
    return -1;
  memcpy(out, d, 64);
  return 0;
}

// the 64-byte-prefix hash the verify path uses (must equal cgs_sha512_prefixed(16, r || ab, ...))
void cgs_sha512_ed25519(const uint32_t* r, const uint32_t* ab, const uint8_t* msg, uint32_t n, uint8_t* out) {
  uint32_t d[16];
  sha512_ed25519(d, r, ab, msg, n);
  memcpy(out, d, 64);
}

// The whole per-element path: key expansion, then the signature over msg[0..n), n > 0.
// msg may have any alignment; the 4-byte words that hold its bytes must be readable.
void cgs_sign(const uint8_t* seed, const uint8_t* msg, uint32_t n, uint8_t* pk, uint8_t* sig) {
  uint32_t sw[8], a[8], prefix[8], ab[8], s[16];
  memcpy(sw, seed, 32);
  ed25519_expand_seed(a, prefix, sw);
  ed25519_public_key(ab, a, get_b);
  ed25519_sign_stage(s, a, prefix, ab, msg, n, get_b);
  memcpy(pk, ab, 32);
  memcpy(sig, s, 64);
}

}  // extern "C"
