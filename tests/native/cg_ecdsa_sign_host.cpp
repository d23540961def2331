// Host build of the device ECDSA signing arithmetic (cg_ecdsa_sign.h: the exact code the
// HIP kernels compile), used only by tests/test_ecdsa_sign_host.py and
// tests/native/ecdsa_sign_san.cpp to check it against the oracle without a GPU.  Built
// twice: -DCG_ECDSA_SIGN_WIN=16 (libcg_ecdsa_sign_host_w16.so) and -DCG_ECDSA_SIGN_WIN=8
// (libcg_ecdsa_sign_host_w8.so, the sanitizer build's window size).  Not part of the product.
#include <stdint.h>
#include <string.h>

#include <unordered_map>

#include "cg_ecdsa_sign.h"

using namespace cg;

namespace {

struct Entry {
  f26 x, y;
};

// the device's per-window tables a 2^(W j) G, each entry built on first use with the
// device's own code (a scalar touches 17 or 33 of them)
template <class C>
void get_t(uint32_t j, uint32_t a, jpt& p) {
  static std::unordered_map<uint32_t, Entry> cache;
  const uint32_t idx = ecdsa_sign_tab_index(j, a);
  auto it = cache.find(idx);
  if (it == cache.end()) {
    Entry e;
    ecdsa_sign_tab_entry<C>(j, a, e.x, e.y);
    it = cache.emplace(idx, e).first;
  }
  p.X = it->second.x;
  p.Y = it->second.y;
  p.inf = 0;
}

void be32_to_limbs(uint32_t out[8], const uint8_t* be) {
  for (int i = 0; i < 8; ++i)
    out[i] = (uint32_t)be[28 - 4 * i] << 24 | (uint32_t)be[29 - 4 * i] << 16 | (uint32_t)be[30 - 4 * i] << 8 |
             be[31 - 4 * i];
}

void limbs_to_be32(uint8_t* be, const uint32_t in[8]) {
  for (int i = 0; i < 8; ++i)
    for (int b = 0; b < 4; ++b) be[31 - 4 * i - b] = (uint8_t)(in[i] >> (8 * b));
}

template <class C>
uint32_t sign_c(const uint8_t* d_be, const uint8_t* msg, uint32_t n, int mode, const uint8_t* k_be, uint8_t* sig,
                uint32_t* sig_len) {
  uint32_t d[8], kc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, len = 0;
  be32_to_limbs(d, d_be);
  if (k_be) be32_to_limbs(kc, k_be);
  memset(sig, 0, 72);
  const uint32_t st = ecdsa_sign_one<C>(d, msg, n, (uint32_t)mode, kc, len, get_t<C>,
                                        [&](uint32_t pos, uint32_t b) { sig[pos] = (uint8_t)b; });
  *sig_len = len;
  return st;
}

template <class C>
void pubkey_c(const uint8_t* d_be, uint8_t* xy) {
  uint32_t d[8], qx[8], qy[8];
  be32_to_limbs(d, d_be);
  ecdsa_sign_pubkey<C>(qx, qy, d, get_t<C>);
  limbs_to_be32(xy, qx);
  limbs_to_be32(xy + 32, qy);
}

}  // namespace

extern "C" {

int cges_win(void) { return kSignWin; }

// The whole per-element path.  d_be, k_be: 32 big-endian bytes (k_be may be null in RFC 6979
// mode); msg may have any alignment and the 4-byte words that hold its bytes must be
// readable; sig: 72 bytes, zero past the signature.  Returns the CG_SIGN_* outcome, or
// 0xff for a scheme that is not 2 or 3.
uint32_t cges_sign(int scheme, const uint8_t* d_be, const uint8_t* msg, uint32_t n, int mode, const uint8_t* k_be,
                   uint8_t* sig, uint32_t* sig_len) {
  if (scheme == 2) return sign_c<CurveK1>(d_be, msg, n, mode, k_be, sig, sig_len);
  if (scheme == 3) return sign_c<CurveR1>(d_be, msg, n, mode, k_be, sig, sig_len);
  return 0xff;
}

// Q = d G as the 64-byte verify key form (X || Y, big-endian)
int cges_pubkey(int scheme, const uint8_t* d_be, uint8_t* xy) {
  if (scheme == 2)
    pubkey_c<CurveK1>(d_be, xy);
  else if (scheme == 3)
    pubkey_c<CurveR1>(d_be, xy);
  else
    return -1;
  return 0;
}

// The RFC 6979 nonce for an arbitrary order above 2^255 (32 big-endian bytes each); h1: the
// message digest.  Returns the number of rejected candidates.
uint32_t cges_rfc6979(const uint8_t* order_be, const uint8_t* d_be, const uint8_t* h1, uint8_t* k_be) {
  uint32_t order[8], d[8], e[8], k[8];
  be32_to_limbs(order, order_be);
  be32_to_limbs(d, d_be);
  be32_to_limbs(e, h1);
  const uint32_t retries = ecdsa_rfc6979_k(k, order, d, e);
  limbs_to_be32(k_be, k);
  return retries;
}

}  // extern "C"
