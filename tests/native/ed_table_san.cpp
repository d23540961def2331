// Stand-alone ASan + UBSan run of the lane-table entry format (cg_ed_table.h): pack and
// unpack at the corners of the pack precondition and on random limb vectors inside it —
// every shift, the 2p offset and the wrap stay free of signed overflow and out-of-range
// accesses — and the round trip keeps the value mod p (f - unpack(pack(f)) == 0).
// Built and run by tests/test_ed_table_format.py; not part of the product.
#include <stdint.h>
#include <stdio.h>

#include "cg_ed_table.h"

using namespace cg;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dull;
}

static int check(const fe& f) {
  uint32_t w[8];
  fe u, d;
  fe_pack_loose(w, f);
  fe_unpack_loose(u, w);
  for (int i = 0; i < 10; ++i) {
    const int32_t top = i == 9 ? (1 << 26) : (i & 1) ? (1 << 25) : (1 << 26);
    if (u.v[i] < 0 || u.v[i] >= top) return 1;
  }
  fe_sub(d, f, u);
  return fe_iszero(d) ? 0 : 2;
}

int main() {
  int bad = 0;
  fe f;
  for (int corner = 0; corner < 1024 && !bad; ++corner) {  // every sign pattern of the extreme limbs
    for (int i = 0; i < 10; ++i) {
      const int32_t m = (1 << ((i & 1) ? 25 : 26)) + kEdPackSlack;
      f.v[i] = (corner >> i) & 1 ? m : -m;
    }
    bad = check(f);
  }
  for (int t = 0; t < 200000 && !bad; ++t) {
    for (int i = 0; i < 10; ++i) {
      const int64_t m = (1LL << ((i & 1) ? 25 : 26)) + kEdPackSlack;
      f.v[i] = (int32_t)((int64_t)(next64() % (uint64_t)(2 * m + 1)) - m);
    }
    bad = check(f);
  }
  uint32_t w[kEdEntryWords];
  ge_cached c;
  ed_entry_identity(w);
  ed_entry_unpack(c, w);
  fe one;
  fe_1(one);
  fe_sub(one, one, c.YplusX);
  if (!bad && !(fe_iszero(one) && c.YminusX.v[0] == 1 && c.Z.v[0] == 1 && fe_iszero(c.T2d))) bad = 3;
  if (bad) {
    fprintf(stderr, "ed_table_san: check %d failed\n", bad);
    return 1;
  }
  printf("ed_table_san ok\n");
  return 0;
}
