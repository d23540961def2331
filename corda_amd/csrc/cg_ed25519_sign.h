// Per-element Ed25519 signing (EDDSA_ED25519_SHA512) with i2p eddsa 0.2.0 / RFC 8032
// semantics: the deterministic signature Crypto.doSign produces for an
// EdDSAPrivateKey (Crypto.kt:394-401 -> EdDSAEngine.engineSign), restated in
// oracle/py/ed25519_i2p.py (seed_to_keypair, sign).
//
//   key expansion  h = SHA-512(seed); a = clamp(h[0..31]) (bits 0-2 and 255 cleared, bit
//                  254 set), prefix = h[32..63]; A = enc([a]B).  a is kept mod L: the
//                  clamped value is >= 2^254, above the recoding's range, and
//                  [a]B = [a mod L]B because B has order L.
//   signature      r = SHA-512(prefix || M) mod L, R = enc([r]B),
//                  k = SHA-512(R || A || M) mod L, S = (r + k a) mod L; sig = R || S.
//
// [k]B for k < L runs over the context's eight shared affine tables T_s[j] = j 2^(32 s) B
// (cg_ed25519.h ed25519_btab_entry): k in signed kBWin-bit digits d_i (sc_recode_b), digit
// i = s (32 / kBWin) + c sits at bit 32 s + kBWin c, so
//   [k]B = sum_c 2^(kBWin c) sum_s d[s (32 / kBWin) + c] T_s
// evaluated as a Horner scheme over the residue classes c: 16 mixed additions and 16
// doublings at kBWin = 16, 32 and 24 at kBWin = 8 — no per-signature table.
// Table loads are indexed by secret digits: not constant-time.
#pragma once
#include "cg_ed25519.h"

namespace cg {

enum : uint32_t { SIGN_OK = 0, SIGN_EMPTY = 1 };  // cordagpu.h CG_SIGN_OK / CG_SIGN_EMPTY

// out = (a b + c) mod L for a, b, c < 2^256.
CG_HD void sc_muladd_mod(uint32_t out[8], const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) {
  uint32_t x[16];
  CG_UNROLL for (int i = 0; i < 8; ++i) {
    x[i] = c[i];
    x[8 + i] = 0;
  }
  CG_UNROLL for (int i = 0; i < 8; ++i) {
    uint64_t cy = 0;
    CG_UNROLL for (int j = 0; j < 8; ++j) {
      const uint64_t t = (uint64_t)a[i] * b[j] + x[i + j] + cy;
      x[i + j] = (uint32_t)t;
      cy = t >> 32;
    }
    x[i + 8] = (uint32_t)cy;  // (word i + 8 is still zero here: no carry is lost)
  }
  sc_reduce512(out, x);
}

// x mod L for a 256-bit x.
CG_HD void sc_reduce256(uint32_t out[8], const uint32_t x[8]) {
  uint32_t w[16];
  CG_UNROLL for (int i = 0; i < 8; ++i) {
    w[i] = x[i];
    w[8 + i] = 0;
  }
  sc_reduce512(out, w);
}

// seed -> (a mod L, prefix).
CG_HD void ed25519_expand_seed(uint32_t a[8], uint32_t prefix[8], const uint32_t seed[8]) {
  uint32_t h[16];
  sha512_prefixed<8>(h, seed, nullptr, 0);  // SHA-512(seed): a 32-byte prefix, no message
  h[0] &= ~7u;
  h[7] = (h[7] & 0x7fffffffu) | 0x40000000u;
  sc_reduce256(a, h);
  CG_UNROLL for (int w = 0; w < 8; ++w) prefix[w] = h[8 + w];
}

// out = [k]B for k < L.  getB(s, j, precomp&) loads j 2^(32 s) B, j <= 2^(kBWin-1)
// (the callback of ed25519_msm); a zero digit adds the tables' identity entry (j = 0).
// The sign of a digit goes into ge_madd's `neg`: no branch depends on a digit.
template <typename GetB>
CG_HD void ed25519_fixed_base(ge_p3& out, const uint32_t k[8], GetB&& getB) {
  static_assert(kBWin == 16 || kBWin == 8, "B digit fields are 8 or 16 bits");
  static_assert(kBTables == 8, "one shared table per 32-bit word of the scalar");
  constexpr int PER = 32 / kBWin;  // digits per 32-bit table step = residue classes
  constexpr uint32_t kMask = (1u << kBWin) - 1, kHalf = 1u << (kBWin - 1);
  uint32_t dig[8];
  sc_recode_b<kBWin>(dig, k);  // digit s PER + c: word 7 - s, field PER - 1 - c
  ge_p1p1 t;
  ge_p2 r2;
  ge_p3 r3;
  ge_precomp pb;
  CG_NOUNROLL for (int c = PER - 1; c >= 0; --c) {
    const uint32_t fsh = (uint32_t)kBWin * (uint32_t)(PER - 1 - c);
    if (c != PER - 1) {
      CG_NOUNROLL for (int b = 0; b < kBWin - 1; ++b) {
        ge_p1p1_to_p2(r2, t);
        ge_p2_dbl<false>(t, r2);
      }
      ge_p1p1_to_p2(r2, t);
      ge_p2_dbl<true>(t, r2);  // the additions follow
    }
    // rolled over the tables; the digit words rotate so every access is static (a runtime
    // index into a register array would go to scratch), back in place after eight steps
    CG_NOUNROLL for (int s = 0; s < kBTables; ++s) {
      const uint32_t e = (dig[7] >> fsh) & kMask;
      const uint32_t top = dig[7];
      CG_UNROLL for (int w = 7; w >= 1; --w) dig[w] = dig[w - 1];
      dig[0] = top;
      const uint32_t neg = e < kHalf;
      getB((uint32_t)s, neg ? kHalf - e : e - kHalf, pb);
      if (c == PER - 1 && s == 0) {
        ge_madd(t, ge_identity_p3(), pb, neg);
      } else {
        ge_p1p1_to_p3<true>(r3, t);
        ge_madd(t, r3, pb, neg);
      }
    }
  }
  ge_p1p1_to_p3(out, t);
}

// enc([k]B), k < L.
template <typename GetB>
CG_HD void ed25519_fixed_base_enc(uint32_t enc[8], const uint32_t k[8], GetB&& getB) {
  ge_p3 P;
  ed25519_fixed_base(P, k, getB);
  ge_tobytes(enc, P.X, P.Y, P.Z);
}

// abyte = enc([a]B), a < L (ed25519_expand_seed's a).
template <typename GetB>
CG_HD void ed25519_public_key(uint32_t abyte[8], const uint32_t a[8], GetB&& getB) {
  ed25519_fixed_base_enc(abyte, a, getB);
}

// sig = R || S over msg[0..n), n > 0 (an empty message is refused before this:
// Crypto.kt:397).  a < L, prefix and abyte from the key expansion.
template <typename GetB>
CG_HD void ed25519_sign_stage(uint32_t sig[16], const uint32_t a[8], const uint32_t prefix[8],
                              const uint32_t abyte[8], const uint8_t* msg, uint32_t n, GetB&& getB) {
  uint32_t hd[16], r[8], k[8];
  sha512_prefixed<8>(hd, prefix, msg, n);
  sc_reduce512(r, hd);
  ed25519_fixed_base_enc(sig, r, getB);  // R: words 0..7
  sha512_ed25519(hd, sig, abyte, msg, n);
  sc_reduce512(k, hd);
  sc_muladd_mod(sig + 8, k, a, r);
}

}  // namespace cg
