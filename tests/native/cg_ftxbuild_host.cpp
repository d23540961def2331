// Host build of the FilteredTransaction builder's device logic (cg_pmt_build.h: the exact
// per-transaction pass the HIP kernel cg_pmt_build compiles, here with the parked hashes in
// a local array instead of an HBM slot; cg_ftx_layout.h: the layout pass of
// cg_ftx_build_batch; cg_sha256.h), used only by tests/test_ftx_build_host.py and
// tests/native/ftxbuild_san.cpp to check it against the oracle without a GPU.  Not part of
// the product.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "cg_ftx_layout.h"
#include "cg_sha256.h"

using namespace cg;

namespace {

struct HostSink {
  const uint32_t* leaves;
  uint32_t k;
  uint32_t parked[33][8];
  uint8_t* kind_out;
  uint8_t* hash_out;
  uint32_t pos, end;
  int overrun = 0;
  uint32_t cur[8];
  void leaf(uint64_t i) {
    for (int q = 0; q < 8; ++q) cur[q] = i < k ? leaves[(size_t)i * 8 + q] : 0u;
  }
  void emit(int kind) {
    if (pos >= end) {
      overrun = 1;
      return;
    }
    kind_out[pos] = (uint8_t)kind;
    for (int q = 0; q < 8; ++q) {
      const uint32_t w = kind == kPmtNode ? 0u : cur[q];
      for (int y = 0; y < 4; ++y) hash_out[(size_t)pos * 32 + 4 * q + y] = (uint8_t)(w >> (24 - 8 * y));
    }
    ++pos;
  }
  void combine(uint32_t l) {
    uint32_t m[16];
    for (int q = 0; q < 8; ++q) {
      m[q] = parked[l][q];
      m[8 + q] = cur[q];
    }
    sha256_words<64>(cur, m);
  }
  void park_hash(uint32_t l) { memcpy(parked[l], cur, 32); }
};

void put_be(uint8_t* dst, const uint32_t* h) {
  for (int q = 0; q < 8; ++q)
    for (int y = 0; y < 4; ++y) dst[4 * q + y] = (uint8_t)(h[q] >> (24 - 8 * y));
}

}  // namespace

extern "C" {

// cg_ftx_build_layout's contract: 0, or -1 (invalid argument)
int cgf_layout(size_t n_tx, const uint32_t* comp_start, const uint8_t* include, uint32_t* fcomp_start_out,
               uint32_t* node_start_out) {
  if (!fcomp_start_out || !node_start_out) return -1;
  FtxBuildLayout lay;
  std::string err;
  if (!ftx_build_layout(n_tx, comp_start, include, lay, err)) return -1;
  memcpy(fcomp_start_out, lay.fstart.data(), 4 * (n_tx + 1));
  memcpy(node_start_out, lay.nstart.data(), 4 * (n_tx + 1));
  return 0;
}

// cg_ftx_build_batch's outputs for a batch in its input layout, sized by cgf_layout (the
// capacities are the start arrays' last entries).  0, -1 for an invalid layout, -2 when a
// transaction's pass does not emit exactly the nodes the layout counted, -3 when the counting
// pass disagrees with the layout's closed form.
int cgf_build(size_t n_tx, const uint8_t* arena, const uint64_t* comp_off, const uint32_t* comp_len,
              const uint32_t* comp_start, const uint8_t* salts, const uint8_t* include, uint32_t* fcomp_start_out,
              uint32_t* fcomp_index_out, uint8_t* nonces_out, uint32_t* node_start_out, uint8_t* node_kind_out,
              uint8_t* node_hash_out, uint8_t* root_out) {
  FtxBuildLayout lay;
  std::string err;
  if (!ftx_build_layout(n_tx, comp_start, include, lay, err)) return -1;
  memcpy(fcomp_start_out, lay.fstart.data(), 4 * (n_tx + 1));
  memcpy(node_start_out, lay.nstart.data(), 4 * (n_tx + 1));
  const uint32_t* pre = lay.inc_prefix.data();
  for (size_t t = 0; t < n_tx; ++t) {
    const uint32_t c0 = comp_start[t], k = comp_start[t + 1] - c0;
    uint32_t sw[9];
    for (int w = 0; w < 8; ++w)
      sw[w] = (uint32_t)salts[32 * t + 4 * w] << 24 | (uint32_t)salts[32 * t + 4 * w + 1] << 16 |
              (uint32_t)salts[32 * t + 4 * w + 2] << 8 | salts[32 * t + 4 * w + 3];
    std::vector<uint32_t> leaves(8 * (size_t)k + 8);
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t c = c0 + i;
      std::vector<uint32_t> pre_image((comp_len[c] + 32 + 3) / 4 + 1);  // word-aligned, whole words
      uint8_t* p = (uint8_t*)pre_image.data();
      if (comp_len[c]) memcpy(p, arena + comp_off[c], comp_len[c]);
      uint32_t n = comp_len[c];
      if (i + 1 < k) {  // every component but the serialized salt carries its nonce
        uint32_t nonce[8];
        sw[8] = i;
        sha256_words<36>(nonce, sw);
        put_be(p + n, nonce);
        n += 32;
        if (pre[c + 1] != pre[c]) {
          fcomp_index_out[pre[c]] = c;
          put_be(nonces_out + 32 * (size_t)pre[c], nonce);
        }
      }
      sha256_mem(&leaves[8 * (size_t)i], p, n);
    }
    // the layout's closed-form count against the pass with the counting sink
    if (pmt_node_count(k, [&](uint32_t i) { return pre[c0 + i]; }) != lay.nstart[t + 1] - lay.nstart[t]) return -3;
    HostSink s;
    s.leaves = leaves.data();
    s.k = k;
    s.kind_out = node_kind_out;
    s.hash_out = node_hash_out;
    s.pos = lay.nstart[t];
    s.end = lay.nstart[t + 1];
    memset(s.cur, 0, 32);
    pmt_walk(k, [&](uint32_t i) { return pre[c0 + i]; }, s);
    if (s.overrun || s.pos != s.end) return -2;
    put_be(root_out + 32 * t, s.cur);
  }
  return 0;
}

}  // extern "C"
