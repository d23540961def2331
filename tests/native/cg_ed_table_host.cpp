// Host build of the lane-table entry format (cg_ed_table.h) and the table builder
// (cg_ed25519.h ed25519_build_table), used only by tests/test_ed_table_format.py: the pack /
// unpack round trip on chosen limb vectors, the builder against the add-only chain it
// replaced, and whole verifies in which every table entry goes through the packed 32 words
// as it does between the points and MSM kernels.  Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "cg_ed25519.h"
#include "cg_ed_table.h"

using namespace cg;

namespace {

struct Packed {
  uint32_t w[kEdEntryWords];
};

// A table of nine entries in storage form: entry 0 is the shared identity entry, the
// others what the points kernels store.
struct PackedTable {
  Packed e[kATabEntries];
  void build(const ge_p3& P) {
    ed25519_build_table(P, [&](int k, const ge_cached& c) {
      if (k) ed_entry_pack(e[k].w, c);
    });
    ed_entry_identity(e[0].w);
  }
  void get(uint32_t k, ge_cached& c) const { ed_entry_unpack(c, e[k].w); }
};

// The builder before the doublings: k P = (k - 1) P + P for every k.
template <typename Put>
void build_table_add_only(const ge_p3& P, Put&& put) {
  ge_cached c;
  fe_1(c.YplusX);
  fe_1(c.YminusX);
  fe_1(c.Z);
  fe_0(c.T2d);
  put(0, c);
  ge_p3_to_cached(c, P);
  put(1, c);
  ge_p1p1 t;
  ge_p2 unused;
  for (int k = 2; k < kATabEntries; ++k) {
    ge_add_cached(t, P, c, 0);
    ge_p1p1_to_cached(c, unused, t);
    put(k, c);
  }
}

void limbs_out(int32_t* out, const ge_cached& c) {
  const fe* f[4] = {&c.YplusX, &c.YminusX, &c.Z, &c.T2d};
  for (int i = 0; i < 4; ++i)
    for (int l = 0; l < 10; ++l) out[10 * i + l] = f[i]->v[l];
}

// the shared tables k * 2^(32 s) B, each entry on first use (as tests/native/cg_host.cpp)
ge_precomp g_btab_store[kBTables][kBTabEntries];
uint8_t g_btab_built[kBTables][kBTabEntries];
void get_b(uint32_t s, uint32_t k, ge_precomp& p) {
  if (!g_btab_built[s][k]) {
    ed25519_btab_entry(g_btab_store[s][k], s, k);
    g_btab_built[s][k] = 1;
  }
  p = g_btab_store[s][k];
}

template <int LANES>
int verify_lanes(const uint32_t pk[8], const uint32_t sig[16], uint32_t sig_len, const uint8_t* msg, uint32_t msg_len,
                 uint32_t mode, uint32_t force_ndig) {
  constexpr int P = LANES / 2, D = 32 / P;
  uint32_t dig[kDigitWords], ndig, rneg;
  uint32_t pre = ed25519_hash_stage(pk, sig, sig_len, msg, msg_len, mode, dig, ndig, rneg);
  ge_p3 A, R;
  pre = ed25519_points_stage(pk, sig, pre, A, R);
  if (pre != V_COMPUTE) return (int)pre;
  static PackedTable tab[LANES];
  for (int q = 0; q < LANES; ++q) {
    ge_p3 pt = q / P ? R : A;
    if (q % P) ge_p3_dbl_n(pt, 4 * D * (q % P));
    tab[q].build(pt);
  }
  if (force_ndig > ndig) ndig = force_ndig;
  ge_p1p1 t[LANES];
  for (uint32_t q = 0; q < LANES; ++q)
    ed25519_msm_lane<Packed, LANES>(
        t[q], ndig, q, [&](int w) { return dig[w]; }, (q / P) ? rneg : 0u,
        [&](uint32_t k, Packed& r) { r = tab[q].e[k]; }, [&](const Packed& r, ge_cached& c) { ed_entry_unpack(c, r.w); },
        get_b);
  for (int m = 1; m < LANES / 2; m *= 2) {
    ge_p1p1 s[LANES];
    for (int q = 0; q < LANES; ++q) {
      ge_p3 x;
      ge_p1p1_to_p3(x, t[q ^ m]);
      const fe* src[4] = {&x.X, &x.Y, &x.Z, &x.T};
      int c = 0;
      s[q] = t[q];
      ed25519_lane_sum(s[q], [&](fe& v) { v = *src[c++]; });
    }
    for (int q = 0; q < LANES; ++q) t[q] = s[q];
  }
  uint32_t ok[LANES];
  for (int q = 0; q < LANES; ++q) {
    ge_p3 x;
    ge_p1p1_to_p3(x, t[q ^ (LANES / 2)]);
    const fe* src[4] = {&x.X, &x.Y, &x.Z, &x.T};
    int c = 0;
    ok[q] = ed25519_pair_combine(t[q], [&](fe& v) { v = *src[c++]; });
  }
  for (int q = 1; q < LANES; ++q)
    if (ok[q] != ok[0]) return -1;
  return ok[0] ? (int)V_ACCEPT : (int)V_REJECT;
}

}  // namespace

extern "C" {

// limbs -> pack -> words, words -> unpack -> limbs
void cgt_pack(const int32_t* limbs, uint32_t* words) {
  fe f;
  for (int i = 0; i < 10; ++i) f.v[i] = limbs[i];
  fe_pack_loose(words, f);
}
void cgt_unpack(const uint32_t* words, int32_t* limbs) {
  fe f;
  fe_unpack_loose(f, words);
  for (int i = 0; i < 10; ++i) limbs[i] = f.v[i];
}
// the identity entry, unpacked: 4 x 10 limbs
void cgt_identity(int32_t* limbs) {
  uint32_t w[kEdEntryWords];
  ed_entry_identity(w);
  ge_cached c;
  ed_entry_unpack(c, w);
  limbs_out(limbs, c);
}
int32_t cgt_pack_slack() { return kEdPackSlack; }

// Decodes enc (i2p rules), optionally negates it as the points kernels negate A, and
// builds k P, k = 0..8, with the builder (after a pack / unpack round trip when `packed`)
// and with the add-only chain: 9 x 40 limbs each.  Returns 0 when enc has no square root.
int cgt_tables(const uint8_t* enc, int negate, int packed, int32_t* out_new, int32_t* out_add) {
  uint32_t w[8];
  memcpy(w, enc, 32);
  ge_p3 P;
  if (!ge_frombytes_i2p(P, w)) return 0;
  if (negate) {
    fe_neg_p(P.X, P.X);
    fe_neg_p(P.T, P.T);
  }
  if (packed) {
    PackedTable t;
    t.build(P);
    for (int k = 0; k < kATabEntries; ++k) {
      ge_cached c;
      t.get(k, c);
      limbs_out(out_new + 40 * k, c);
    }
  } else {
    ed25519_build_table(P, [&](int k, const ge_cached& c) { limbs_out(out_new + 40 * k, c); });
  }
  build_table_add_only(P, [&](int k, const ge_cached& c) { limbs_out(out_add + 40 * k, c); });
  return 1;
}

// The balanced path: hash -> points -> tables (packed) -> msm, one lane.
int cgt_verify(const uint8_t* pk_bytes, const uint8_t* sig_bytes, uint32_t sig_len, const uint8_t* msg, uint32_t msg_len,
               uint32_t mode, uint32_t force_ndig) {
  uint32_t pk[8], sig[16] = {0};
  memcpy(pk, pk_bytes, 32);
  memcpy(sig, sig_bytes, sig_len < 64 ? sig_len : 64);
  uint32_t dig[kDigitWords], ndig, rneg;
  uint32_t pre = ed25519_hash_stage(pk, sig, sig_len, msg, msg_len, mode, dig, ndig, rneg);
  ge_p3 negA, R;
  pre = ed25519_points_stage(pk, sig, pre, negA, R);
  if (pre != V_COMPUTE) return (int)pre;
  PackedTable ta, tr;
  ta.build(negA);
  tr.build(R);
  if (force_ndig > ndig) ndig = force_ndig;
  const uint32_t ok = ed25519_msm<Packed, Packed>(
      ndig, [&](int w) { return dig[w]; }, rneg, [&](uint32_t k, Packed& r) { r = ta.e[k]; },
      [&](const Packed& r, ge_cached& c) { ed_entry_unpack(c, r.w); }, [&](uint32_t k, Packed& r) { r = tr.e[k]; },
      [&](const Packed& r, ge_cached& c) { ed_entry_unpack(c, r.w); }, get_b);
  return ok ? (int)V_ACCEPT : (int)V_REJECT;
}

// The latency mode with 2, 4 or 8 lanes per signature; -1 when the lanes disagree.
int cgt_verify_lanes(int lanes, const uint8_t* pk_bytes, const uint8_t* sig_bytes, uint32_t sig_len, const uint8_t* msg,
                     uint32_t msg_len, uint32_t mode, uint32_t force_ndig) {
  uint32_t pk[8], sig[16] = {0};
  memcpy(pk, pk_bytes, 32);
  memcpy(sig, sig_bytes, sig_len < 64 ? sig_len : 64);
  return lanes == 2   ? verify_lanes<2>(pk, sig, sig_len, msg, msg_len, mode, force_ndig)
         : lanes == 4 ? verify_lanes<4>(pk, sig, sig_len, msg, msg_len, mode, force_ndig)
                      : verify_lanes<8>(pk, sig, sig_len, msg, msg_len, mode, force_ndig);
}

// The key-reuse path: per-key tables (packed) -> hash<REUSE> -> points_r -> R table
// (packed) -> msm_reuse.
int cgt_verify_reuse(const uint8_t* pk_bytes, const uint8_t* sig_bytes, uint32_t sig_len, const uint8_t* msg,
                     uint32_t msg_len, uint32_t mode, uint32_t wide) {
  uint32_t pk[8], sig[16] = {0};
  memcpy(pk, pk_bytes, 32);
  memcpy(sig, sig_bytes, sig_len < 64 ? sig_len : 64);
  static Packed kt[4][kATabEntries];
  // (cg_ed25519_keyprep packs entry 0, the identity, like the others)
  const uint32_t key_ok = ed25519_key_tables(pk, [&](int t, int k, const ge_cached& c) { ed_entry_pack(kt[t][k].w, c); });
  uint32_t dig[kDigitWords], w, rneg;
  uint32_t pre = ed25519_hash_stage<false, true>(pk, sig, sig_len, msg, msg_len, mode, dig, w, rneg);
  ge_p3 R;
  pre = ed25519_points_stage_r(sig, pre, key_ok, R);
  if (pre != V_COMPUTE) return (int)pre;
  PackedTable tr;
  tr.build(R);
  const uint32_t ok = ed25519_msm_reuse(
      wide ? 16u : (w & 31u), wide ? 1u : (w >> 5), dig, rneg,
      [&](uint32_t t, uint32_t k, ge_cached& c) { ed_entry_unpack(c, kt[t][k].w); },
      [&](uint32_t k, ge_cached& c) { tr.get(k, c); }, get_b);
  return ok ? (int)V_ACCEPT : (int)V_REJECT;
}

#if defined(CG_CHECK_BOUNDS)
void cgt_bounds_report(int64_t* max_limb, double* log2_max_col) {
  *max_limb = cg_bounds().max_limb;
  *log2_max_col = __builtin_log2((double)cg_bounds().max_col);
}
#endif
}
