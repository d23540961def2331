// The storage format of a per-signature (lane) or per-key table entry of the Ed25519
// verify kernels: one cached point (Y+X, Y-X, Z, 2dT) in 32 words = one 128-byte line.
// The points kernels pack (ed_entry_pack), the MSM kernels unpack (ed_entry_unpack); the
// host tests compile the same functions (tests/native/cg_ed_table_host.cpp).
//
// A coordinate is stored as a 256-bit value V in 8 little-endian words, V = the field
// element mod p but NOT reduced: limbs 0..8 brought into [0, 2^w) and limb 9 into
// [0, 2^26) by one floor carry chain, so V < 2^256 and bit 255 is part of the value (the
// MSM only multiplies by an entry; the accept test is made on the accumulator, never on a
// table entry, so no canonical form is needed).  Word layout: limb i starts at bit
// ceil(25.5 i) as in fe_tobytes; limb 9 takes bits 230..255.
//
//   pack    precondition: every limb |f_i| <= 2^w + 2^24 (w = 26 / 25 for even / odd i) —
//           floor-shaped products (limb 1 within 2^16 of [0, 2^25)), their differences
//           Y - X and corrected sums Y + X - p (|limb| <= 2^w + 2^16), proved for the table
//           builder by tests/test_fe_intervals_table.py.
//           + 2p limb by limb (all limbs positive: >= 2^w - 2^24 - 38), the part of limb 9
//           above 25 bits (<= 3) wrapped x19 into limb 0, one floor chain 0 -> 9 (carries
//           <= 3): limbs 0..8 in [0, 2^w), limb 9 <= 2^25 + 2.
//   unpack  limbs 0..8 in [0, 2^w), limb 9 in [0, 2^26): inside what the MSM's prescales
//           allow (19 x 2^26 < 2^31), same proof.
#pragma once
#include "cg_ge25519.h"

namespace cg {

constexpr int kEdEntryWords = 32;                  // 4 coordinates x 8 words
constexpr int32_t kEdPackSlack = 1 << 24;          // pack precondition: |limb i| <= 2^w + kEdPackSlack

CG_HD void fe_pack_loose(uint32_t w[8], const fe& f) {
  uint32_t u[10];
  CG_UNROLL for (int i = 0; i < 10; ++i) {
    const int32_t p = i == 0 ? (1 << 26) - 19 : (i & 1) ? (1 << 25) - 1 : (1 << 26) - 1;
#if defined(CG_CHECK_BOUNDS) && !defined(__HIP_DEVICE_COMPILE__)
    const int64_t lim = (1LL << ((i & 1) ? 25 : 26)) + kEdPackSlack, a = f.v[i] < 0 ? -(int64_t)f.v[i] : f.v[i];
    if (a > lim) {
      fprintf(stderr, "cg bounds: packed limb %d = %lld outside the pack precondition\n", i, (long long)f.v[i]);
      __builtin_trap();
    }
#endif
    u[i] = (uint32_t)(f.v[i] + 2 * p);
  }
  u[0] += 19u * (u[9] >> 25);
  u[9] &= 0x1ffffffu;
  CG_UNROLL for (int i = 0; i < 9; ++i) {
    const int sh = (i & 1) ? 25 : 26;
    u[i + 1] += u[i] >> sh;
    u[i] &= (1u << sh) - 1;
  }
  w[0] = u[0] | u[1] << 26;
  w[1] = u[1] >> 6 | u[2] << 19;
  w[2] = u[2] >> 13 | u[3] << 13;
  w[3] = u[3] >> 19 | u[4] << 6;
  w[4] = u[5] | u[6] << 25;
  w[5] = u[6] >> 7 | u[7] << 19;
  w[6] = u[7] >> 13 | u[8] << 12;
  w[7] = u[8] >> 20 | u[9] << 6;
}

// The inverse word layout; unlike fe_frombytes (the i2p decode, which must drop bit 255)
// limb 9 keeps all 26 bits.
CG_HD void fe_unpack_loose(fe& h, const uint32_t w[8]) {
  h.v[0] = (int32_t)(w[0] & 0x3ffffff);
  h.v[1] = (int32_t)((w[0] >> 26 | w[1] << 6) & 0x1ffffff);
  h.v[2] = (int32_t)((w[1] >> 19 | w[2] << 13) & 0x3ffffff);
  h.v[3] = (int32_t)((w[2] >> 13 | w[3] << 19) & 0x1ffffff);
  h.v[4] = (int32_t)((w[3] >> 6) & 0x3ffffff);
  h.v[5] = (int32_t)(w[4] & 0x1ffffff);
  h.v[6] = (int32_t)((w[4] >> 25 | w[5] << 7) & 0x3ffffff);
  h.v[7] = (int32_t)((w[5] >> 19 | w[6] << 13) & 0x1ffffff);
  h.v[8] = (int32_t)((w[6] >> 12 | w[7] << 20) & 0x3ffffff);
  h.v[9] = (int32_t)(w[7] >> 6);
}

CG_HD void ed_entry_pack(uint32_t w[kEdEntryWords], const ge_cached& c) {
  fe_pack_loose(w, c.YplusX);
  fe_pack_loose(w + 8, c.YminusX);
  fe_pack_loose(w + 16, c.Z);
  fe_pack_loose(w + 24, c.T2d);
}

CG_HD void ed_entry_unpack(ge_cached& c, const uint32_t w[kEdEntryWords]) {
  fe_unpack_loose(c.YplusX, w);
  fe_unpack_loose(c.YminusX, w + 8);
  fe_unpack_loose(c.Z, w + 16);
  fe_unpack_loose(c.T2d, w + 24);
}

// The identity (1, 1, 1, 0) in the entry format, as eight 4-word quads (the device's
// shared identity entry is initialised from the same list).
#define CG_ED_IDENT_QUADS \
  {1, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}
CG_HD void ed_entry_identity(uint32_t w[kEdEntryWords]) {
  const uint32_t q[kEdEntryWords / 4][4] = {CG_ED_IDENT_QUADS};
  CG_UNROLL for (int i = 0; i < kEdEntryWords; ++i) w[i] = q[i / 4][i % 4];
}

}  // namespace cg
