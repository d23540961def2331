// Host-only: the output layout of cg_ftx_build_batch (cordagpu.cpp; also compiled into the
// CPU test build, tests/native/cg_ftxbuild_host.cpp).  Every failure is an invalid argument:
// false, with the reason in `err`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "cg_pmt_build.h"

namespace cg {

// Output layout of cg_ftx_build_batch: a function of the component counts and the include
// mask only, computed on the host (cg_pmt_build.h: pmt_node_count_mask, the closed form of
// the length of the program the kernel's pass emits).  inc_prefix[c] = included components before component c of the batch
// (n_comp + 1 entries) — both the kernel's included-below test and, for an included c,
// its position among the filtered components.
struct FtxBuildLayout {
  std::vector<uint32_t> inc_prefix, fstart, nstart;
  uint32_t max_k = 0;
  bool any_empty = false;
};

inline bool ftx_build_layout(size_t n_tx, const uint32_t* comp_start, const uint8_t* include, FtxBuildLayout& lay,
                           std::string& err) {
  if (n_tx > 0xFFFFFFF0ull) return err = "too many transactions", false;
  if (!comp_start) return err = "null pointer", false;
  for (size_t t = 0; t < n_tx; ++t)
    if (comp_start[t + 1] < comp_start[t]) return err = "comp_start not monotone", false;
  const size_t c_begin = comp_start[0], n_comp = comp_start[n_tx];
  if (n_comp > c_begin && !include) return err = "null pointer", false;
  lay.inc_prefix.assign(n_comp + 1, 0);
  lay.fstart.assign(n_tx + 1, 0);
  lay.nstart.assign(n_tx + 1, 0);
  uint32_t* pre = lay.inc_prefix.data();
  for (size_t c = c_begin; c < n_comp; ++c) pre[c + 1] = pre[c] + (include[c] != 0);
  uint64_t nodes = 0;
  for (size_t t = 0; t < n_tx; ++t) {
    const uint32_t c0 = comp_start[t], k = comp_start[t + 1] - c0;
    // the privacy salt is never a filtered component (MerkleTransaction.kt:112-117)
    if (k && include[c0 + k - 1])
      return err = "the include mask selects the privacy salt (last component) of transaction " + std::to_string(t),
             false;
    lay.any_empty |= k == 0;
    lay.max_k = std::max(lay.max_k, k);
    nodes += pmt_node_count_mask(include + c0, k);
    if (nodes > 0xFFFFFFFFull) return err = "more than 2^32 - 1 partial tree nodes", false;
    lay.fstart[t + 1] = pre[c0 + k];
    lay.nstart[t + 1] = (uint32_t)nodes;
  }
  return true;
}

}  // namespace cg
