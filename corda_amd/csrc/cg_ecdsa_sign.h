// Per-element ECDSA signing (ECDSA_SECP256K1_SHA256, ECDSA_SECP256R1_SHA256) with
// BouncyCastle 1.57 semantics: what Crypto.doSign produces for an EC private key
// (Crypto.kt:394-401 -> DSABase.engineSign -> ECDSASigner.generateSignature -> StdDSAEncoder),
// as a pure function of (d, e, k), restated in oracle/py/ecdsa_bc.py (rfc6979_k, sign_rs,
// der_encode):
//
//   e = SHA-256(M) as a 256-bit integer
//   k   RFC 6979 §3.2 (HMAC-SHA-256, qlen = hlen = 256) from (d, e mod n), or the caller's
//   r = x(k G) mod n,  s = k^-1 (e + d r) mod n;  r = 0 or s = 0: BC would draw k again
//   sig = 30 L 02 Lr r 02 Ls s, minimal (the inverse of der_parse, cg_ecdsa.h)
//
// k G is a fixed-base multiplication with no doublings: k in signed kSignWin-bit digits
// d_j (j = 0 .. 256 / kSignWin - 1) plus the recoding's carry out of the top window (both
// orders start 0xFFFF..., so a top window of all ones is reachable) as one more digit
// (0 or 1) at 2^256, over per-window tables T_j[a] = a 2^(kSignWin j) G (affine, Montgomery
// limbs, the one-line entry format of the verifier's G table):
//   k G = sum_j sign(d_j) T_j[|d_j|]  (+ T_top[1] when the carry is set)
// 17 mixed additions at kSignWin = 16 (16 tables of 2^15 + 1 entries, 67 MB per curve), 33
// at kSignWin = 8 (32 tables of 129 entries, 0.5 MB per curve).  Zero digits are skipped
// and the first non-zero digit loads the accumulator (ec_add's exact cases).
// Table loads are indexed by secret digits: not constant-time.
#pragma once
#include "cg_ecdsa.h"

#ifndef CG_ECDSA_SIGN_WIN
#define CG_ECDSA_SIGN_WIN 16  // measured against 8: DESIGN.md §3.8, profiles/ecdsa_sign_mi355x.json
#endif

namespace cg {

// cordagpu.h CG_SIGN_*: per-element outcomes, in order of precedence
enum : uint32_t { ECSIGN_OK = 0, ECSIGN_EMPTY = 1, ECSIGN_NONCE_INVALID = 2, ECSIGN_DEGENERATE = 3 };
enum : uint32_t { ECNONCE_RFC6979 = 0, ECNONCE_CALLER = 1 };

constexpr int kSignWin = CG_ECDSA_SIGN_WIN;
static_assert(kSignWin == 16 || kSignWin == 8, "signing windows are 8 or 16 bits");
constexpr int kSignWins = 256 / kSignWin;                        // tables T_0 .. T_(kSignWins - 1)
constexpr uint32_t kSignHalf = 1u << (kSignWin - 1);             // |digit| <= kSignHalf
constexpr uint32_t kSignTabStride = kSignHalf + 1;               // entries a = 0 (unused, zero) .. kSignHalf
constexpr uint32_t kSignTabEntries = kSignWins * kSignTabStride + 2;  // + the carry's table: a = 0, 1 at 2^256
constexpr int kSignEntryWords = 32;                              // x | y (20 words) padded to a 128-byte line

// Entry (j, a) of the tables: index j * kSignTabStride + a (j = kSignWins: the carry digit).
CG_HD uint32_t ecdsa_sign_tab_index(uint32_t j, uint32_t a) { return j * kSignTabStride + a; }

// Affine a 2^(kSignWin j) G in Montgomery form, 1 <= a <= kSignHalf, j <= kSignWins: a G by
// left-to-right binary with the exact formulas, kSignWin j doublings, one inversion.  One
// lane per entry at the table build (and on the host for the tests).
template <class C>
CG_HD void ecdsa_sign_tab_entry(uint32_t j, uint32_t a, f26& x, f26& y) {
  jpt g, acc;
  ec_generator<C>(g);
  CG_UNROLL for (int i = 0; i < 10; ++i) acc.X.v[i] = acc.Y.v[i] = acc.Z.v[i] = 0;
  acc.inf = 1;
  CG_NOUNROLL for (int b = kSignWin - 1; b >= 0; --b) {
    ec_dbl<C>(acc, acc);
    if ((a >> b) & 1) ec_add<C, true>(acc, acc, g, 0);
  }
  CG_NOUNROLL for (uint32_t i = 0; i < (uint32_t)kSignWin * j; ++i) ec_dbl<C>(acc, acc);
  ec_to_affine<C>(x, y, acc);
}

// Signed radix-2^kSignWin digits of k < 2^256: e = d + kSignHalf, d in [-kSignHalf,
// kSignHalf), in kSignWin-bit fields, digit j in word j / (32 / kSignWin) from the low
// field up; returns the carry out of the top window (the digit at 2^256).
CG_HD uint32_t ecdsa_sign_recode(uint32_t out[8], const uint32_t k[8]) {
  constexpr int PER = 32 / kSignWin;
  constexpr uint32_t kMask = (1u << kSignWin) - 1;
  uint32_t carry = 0;
  CG_UNROLL for (int w = 0; w < 8; ++w) {
    uint32_t o = 0;
    CG_UNROLL for (int f = 0; f < PER; ++f) {
      const uint32_t v = ((k[w] >> (kSignWin * f)) & kMask) + carry;
      carry = v >= kSignHalf;
      o |= ((v + kSignHalf) & kMask) << (kSignWin * f);  // v + half - 2^W carry
    }
    out[w] = o;
  }
  return carry;
}

// acc = k G for k < 2^256 (Jacobian; infinity for k = 0 mod n).  getT(j, a, jpt&) loads the
// affine entry (j, a), 1 <= a <= kSignHalf.  One addition site in a rolled loop; the digit
// words shift so every register access is static.
template <class C, typename GetT>
CG_HD void ecdsa_fixed_base(jpt& acc, const uint32_t k[8], GetT&& getT) {
  constexpr uint32_t kMask = (1u << kSignWin) - 1;
  uint32_t dig[8];
  const uint32_t carry = ecdsa_sign_recode(dig, k);
  CG_UNROLL for (int i = 0; i < 10; ++i) acc.X.v[i] = acc.Y.v[i] = acc.Z.v[i] = 0;
  acc.inf = 1;
  jpt t;
  CG_NOUNROLL for (int j = 0; j <= kSignWins; ++j) {
    const uint32_t e = j == kSignWins ? carry + kSignHalf : dig[0] & kMask;
    CG_UNROLL for (int w = 0; w < 7; ++w) dig[w] = dig[w] >> kSignWin | dig[w + 1] << (32 - kSignWin);
    dig[7] >>= kSignWin;
    const uint32_t neg = e < kSignHalf, a = neg ? kSignHalf - e : e - kSignHalf;
    getT((uint32_t)j, a == 0 ? 1u : a, t);  // (a zero digit loads entry 1 and skips the addition)
    f26 ny;
    f26_neg(ny, t.Y);
    f26_select(t.Y, t.Y, ny, neg);
    t.inf = 0;
    ec_add<C, true>(acc, acc, t, a == 0);
  }
}

// ------------------------------------------------------------------ HMAC-SHA-256
// Keys and messages of RFC 6979 only: a 32-byte key, and messages V (32 bytes),
// V || tag (33) and V || tag || x || h (97).  Values are 8 big-endian-valued words (word 0
// is bytes 0..3), as sha256_mem leaves a digest.
struct hmac256 {
  uint32_t hi[8], ho[8];  // the states after the key's ipad / opad blocks
};

CG_HD void hmac256_key(hmac256& st, const uint32_t key[8]) {
  uint32_t w[16];
  CG_UNROLL for (int j = 0; j < 16; ++j) w[j] = (j < 8 ? key[j] : 0u) ^ 0x36363636u;
  sha256_init(st.hi);
  sha256_block(st.hi, w);
  CG_UNROLL for (int j = 0; j < 16; ++j) w[j] = (j < 8 ? key[j] : 0u) ^ 0x5c5c5c5cu;
  sha256_init(st.ho);
  sha256_block(st.ho, w);
}

// out = H(opad block || inner digest): one more block on the opad state (96 bytes in all)
CG_HD void hmac256_outer(uint32_t out[8], const hmac256& st, const uint32_t inner[8]) {
  uint32_t w[16];
  CG_UNROLL for (int j = 0; j < 16; ++j) w[j] = j < 8 ? inner[j] : 0u;
  w[8] = 0x80000000u;
  w[15] = 96 * 8;
  CG_UNROLL for (int j = 0; j < 8; ++j) out[j] = st.ho[j];
  sha256_block(out, w);
}

// out = HMAC(key, V)
CG_HD void hmac256_v(uint32_t out[8], const hmac256& st, const uint32_t v[8]) {
  uint32_t h[8], w[16];
  CG_UNROLL for (int j = 0; j < 16; ++j) w[j] = j < 8 ? v[j] : 0u;
  w[8] = 0x80000000u;
  w[15] = (64 + 32) * 8;
  CG_UNROLL for (int j = 0; j < 8; ++j) h[j] = st.hi[j];
  sha256_block(h, w);
  hmac256_outer(out, st, h);
}

// out = HMAC(key, V || tag)
CG_HD void hmac256_v_tag(uint32_t out[8], const hmac256& st, const uint32_t v[8], uint32_t tag) {
  uint32_t h[8], w[16];
  CG_UNROLL for (int j = 0; j < 16; ++j) w[j] = j < 8 ? v[j] : 0u;
  w[8] = tag << 24 | 0x00800000u;
  w[15] = (64 + 33) * 8;
  CG_UNROLL for (int j = 0; j < 8; ++j) h[j] = st.hi[j];
  sha256_block(h, w);
  hmac256_outer(out, st, h);
}

// out = HMAC(key, V || tag || x || h): 97 bytes, x and h one byte off the word grid
CG_HD void hmac256_v_tag_xh(uint32_t out[8], const hmac256& st, const uint32_t v[8], uint32_t tag, const uint32_t x[8],
                            const uint32_t h1[8]) {
  uint32_t h[8], w[16];
  CG_UNROLL for (int j = 0; j < 8; ++j) h[j] = st.hi[j];
  // words 8..15 of the message: tag, then x shifted by one byte
  CG_UNROLL for (int j = 0; j < 8; ++j) {
    w[j] = v[j];
    w[8 + j] = (j == 0 ? tag << 24 : x[j - 1] << 24) | x[j] >> 8;
  }
  sha256_block(h, w);
  // words 16..24: the last byte of x, h shifted by one byte, its last byte and the padding marker
  CG_UNROLL for (int j = 0; j < 8; ++j) w[j] = (j == 0 ? x[7] << 24 : h1[j - 1] << 24) | h1[j] >> 8;
  w[8] = h1[7] << 24 | 0x00800000u;
  CG_UNROLL for (int j = 9; j < 15; ++j) w[j] = 0;
  w[15] = (64 + 97) * 8;
  sha256_block(h, w);
  hmac256_outer(out, st, h);
}

// RFC 6979 §3.2 nonce for qlen = hlen = 256: oracle/py/ecdsa_bc.py rfc6979_k(order, d, h1).
// d < order and the result as 8 LE limbs; e: the digest as a 256-bit integer (8 LE limbs),
// reduced here with one conditional subtraction (any order above 2^255, so the tests can
// drive the retry loop with an artificial one).  Returns the number of rejected candidates.
CG_HD uint32_t ecdsa_rfc6979_k(uint32_t k[8], const uint32_t order[8], const uint32_t d[8], const uint32_t e[8]) {
  uint32_t x[8], h1[8], t[8], V[8], K[8];
  const uint32_t bw = mp_sub(t, e, order);
  mp_select(t, t, e, bw);  // e mod order
  CG_UNROLL for (int i = 0; i < 8; ++i) {
    x[i] = d[7 - i];
    h1[i] = t[7 - i];
    V[i] = 0x01010101u;
    K[i] = 0;
  }
  hmac256 st;
  hmac256_key(st, K);
  hmac256_v_tag_xh(K, st, V, 0x00, x, h1);
  hmac256_key(st, K);
  hmac256_v(V, st, V);
  hmac256_v_tag_xh(K, st, V, 0x01, x, h1);
  hmac256_key(st, K);
  hmac256_v(V, st, V);
  uint32_t retries = 0;
  while (true) {
    hmac256_v(V, st, V);
    CG_UNROLL for (int i = 0; i < 8; ++i) k[i] = V[7 - i];
    if (!mp_iszero(k) && mp_lt(k, order)) break;
    ++retries;
    hmac256_v_tag(K, st, V, 0x00);
    hmac256_key(st, K);
    hmac256_v(V, st, V);
  }
  return retries;
}

// ------------------------------------------------------------------ the sign stage
// Front half, one element: the outcome so far (ECSIGN_OK: go on), e mod n, the nonce k in
// [1, n-1] and R = k G (Jacobian).  kc: the caller's nonce (8 LE limbs; CALLER mode).
// The message is not read when it is empty.
template <class C, typename GetT>
CG_HD uint32_t ecdsa_sign_front(const uint32_t d[8], const uint8_t* msg, uint32_t msg_len, uint32_t nonce_mode,
                                const uint32_t kc[8], uint32_t e[8], uint32_t k[8], jpt& R, GetT&& getT) {
  if (msg_len == 0) return ECSIGN_EMPTY;  // Crypto.kt:397
  uint32_t hbe[8], nn[8], t[8];
  C::n(nn);
  sha256_mem(hbe, msg, msg_len);
  CG_UNROLL for (int i = 0; i < 8; ++i) e[i] = hbe[7 - i];
  if (nonce_mode == ECNONCE_CALLER) {
    CG_UNROLL for (int i = 0; i < 8; ++i) k[i] = kc[i];
    if (mp_iszero(k) || !mp_lt(k, nn)) return ECSIGN_NONCE_INVALID;  // RandomDSAKCalculator.nextK draws again
  } else {
    ecdsa_rfc6979_k(k, nn, d, e);
  }
  const uint32_t bw = mp_sub(t, e, nn);
  mp_select(e, t, e, bw);  // e mod n (e < 2^256 < 2n)
  ecdsa_fixed_base<C>(R, k, getT);
  return ECSIGN_OK;
}

// Back half: r = x(R) mod n from X and Z^-1 (Montgomery form), s = k^-1 (e + d r) mod n
// from k^-1 in the Montgomery domain mod n (k^-1 2^256, what the batched inversion leaves).
template <class C>
CG_HD uint32_t ecdsa_sign_finish(const uint32_t d[8], const uint32_t e[8], const f26& X, const f26& zinv,
                                 const uint32_t kinv_m[8], uint32_t r[8], uint32_t s[8]) {
  f26 zi2, xa;
  uint32_t nn[8], x[8], t[8], u[8];
  C::n(nn);
  f26_sqr<C>(zi2, zinv);
  f26_mul<C>(xa, X, zi2);
  f26_to_u256<C>(x, xa);
  const uint32_t bw = mp_sub(t, x, nn);
  mp_select(r, t, x, bw);  // x mod n (x < p < 2n)
  if (mp_iszero(r)) return ECSIGN_DEGENERATE;
  mn_mulmod<C>(t, d, r);  // d r
  const uint32_t cy = mp_add(u, t, e);
  mp_sub(t, u, nn);
  mp_select(u, u, t, cy | !mp_lt(u, nn));  // e + d r mod n
  mn_mul<C>(s, kinv_m, u);                   // k^-1 R (e + d r) R^-1
  if (mp_iszero(s)) return ECSIGN_DEGENERATE;
  return ECSIGN_OK;
}

// StdDSAEncoder.encode: 30 L 02 Lr r 02 Ls s with minimal INTEGERs (0 < r, s < 2^256), 8 to
// 72 bytes; put(pos, byte) for every byte, in order of position inside each part.  The
// source bytes are taken at static positions; only the destination moves.
template <typename Put>
CG_HD uint32_t ecdsa_der_encode(const uint32_t r[8], const uint32_t s[8], Put&& put) {
  const uint32_t lr = mp_bitlen256(r) / 8 + 1, ls = mp_bitlen256(s) / 8 + 1;  // a 0x00 pad when the top bit is set
  put(0u, 0x30u);
  put(1u, 4 + lr + ls);
  put(2u, 0x02u);
  put(3u, lr);
  put(4 + lr, 0x02u);
  put(5 + lr, ls);
  CG_UNROLL for (uint32_t q = 0; q < 33; ++q) {  // byte q of 0x00 || the 32 big-endian bytes
    const uint32_t br = q == 0 ? 0u : (r[7 - (q - 1) / 4] >> (8 * (3 - (q - 1) % 4))) & 0xffu;
    const uint32_t bs = q == 0 ? 0u : (s[7 - (q - 1) / 4] >> (8 * (3 - (q - 1) % 4))) & 0xffu;
    if (q + lr >= 33) put(4 + q + lr - 33, br);
    if (q + ls >= 33) put(6 + lr + q + ls - 33, bs);
  }
  return 6 + lr + ls;
}

// Q = d G as affine (x, y), 8 LE limbs each (key expansion; 0 < d < n).
template <class C, typename GetT>
CG_HD void ecdsa_sign_pubkey(uint32_t qx[8], uint32_t qy[8], const uint32_t d[8], GetT&& getT) {
  jpt Q;
  f26 x, y;
  ecdsa_fixed_base<C>(Q, d, getT);
  ec_to_affine<C>(x, y, Q);
  f26_to_u256<C>(qx, x);
  f26_to_u256<C>(qy, y);
}

// One element on its own (host tests; the kernels take both inversions from the chunk's
// product trees): the outcome, and for ECSIGN_OK the signature bytes through put; returns
// the length through sig_len (0 unless OK).
template <class C, typename GetT, typename Put>
CG_HD uint32_t ecdsa_sign_one(const uint32_t d[8], const uint8_t* msg, uint32_t msg_len, uint32_t nonce_mode,
                              const uint32_t kc[8], uint32_t& sig_len, GetT&& getT, Put&& put) {
  uint32_t e[8], k[8], kinv[8], r2[8], r[8], s[8];
  jpt R;
  sig_len = 0;
  uint32_t st = ecdsa_sign_front<C>(d, msg, msg_len, nonce_mode, kc, e, k, R, getT);
  if (st != ECSIGN_OK) return st;
  f26 zi;
  f26_inv<C>(zi, R.Z);
  mn_inv<C>(kinv, k);
  mn_r2<C>(r2);
  mn_mul<C>(kinv, kinv, r2);  // into the Montgomery domain
  st = ecdsa_sign_finish<C>(d, e, R.X, zi, kinv, r, s);
  if (st != ECSIGN_OK) return st;
  sig_len = ecdsa_der_encode(r, s, put);
  return ECSIGN_OK;
}

}  // namespace cg
