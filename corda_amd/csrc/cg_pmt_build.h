// Per-transaction logic of cg_ftx_build_batch: FilteredTransaction.buildMerkleTransaction
// (MerkleTransaction.kt:159-166) -> PartialMerkleTree.build (PartialMerkleTree.kt:66-123)
// over the full tree of MerkleTree.getMerkleTree (MerkleTree.kt:27-66), as one depth-first
// pass that visits every node of the padded tree once, in post-order, and says for each
// what it contributes to the partial tree's post-order node program.
//
// Inclusion is by component INDEX.  The JVM includes by hash value (`root.hash in
// includeHashes`); the two agree because distinct indices of a transaction give distinct
// nonces, hence distinct leaf hashes.  The privacy salt (last component) can never be in
// FilteredLeaves (MerkleTransaction.kt:112-117) and pad leaves are never included, so
// `require(zeroHash !in includeHashes)` cannot fire.
//
// Host + device (CG_HD) and free of hashing: the caller's sink owns the running hash.  The
// kernel (merkle_kernels.hip: cg_pmt_build), the host-side layout pass (cordagpu.cpp:
// cg_ftx_build_layout) and the CPU test build (tests/native/cg_ftxbuild_host.cpp) all run
// exactly this code.
#pragma once
#include "cg_common.h"

namespace cg {

// PartialTree node kinds of the post-order program (cg_ftx_verify_batch's input format)
enum : uint8_t { kPmtIncluded = 0, kPmtLeaf = 1, kPmtNode = 2 };

// levels above the leaves of a tx with k components: the padded leaf count is 2^L >= k
CG_HD uint32_t pmt_levels(uint32_t k) {
  uint32_t L = 0;
  while (((uint64_t)1 << L) < k) ++L;
  return L;
}

// Is an included component below node idx of level l (leaves [idx 2^l, (idx + 1) 2^l))?
// inc(i), 0 <= i <= k: the number of included components among the tx's first i (any
// common offset cancels).  Positions >= k are padding.
template <class Inc>
CG_HD bool pmt_has(Inc&& inc, uint32_t k, uint32_t l, uint64_t idx) {
  const uint64_t a = idx << l;  // l <= 32, idx 2^l <= 2^32
  uint64_t b = (idx + 1) << l;
  if (a >= k) return false;
  if (b > k) b = k;
  return inc((uint32_t)b) != inc((uint32_t)a);
}

// What the finished subtree (l, idx) appends to the program (PartialMerkleTree.kt:98-123):
// an included leaf is IncludedLeaf; an inner node with an included leaf below is Node (its
// two subtrees are already in the program); a subtree without one is cut to a single
// Leaf(its hash) — which is in the program only when its parent is a Node, i.e. when the
// sibling subtree holds an included leaf, or when it is the root.  -1: nothing.
template <class Inc>
CG_HD int pmt_emit_kind(Inc&& inc, uint32_t k, uint32_t L, uint32_t l, uint64_t idx) {
  if (pmt_has(inc, k, l, idx)) return l == 0 ? kPmtIncluded : kPmtNode;
  if (l == L || pmt_has(inc, k, l, idx ^ 1)) return kPmtLeaf;
  return -1;
}

// The pass.  The sink keeps one running hash `cur` and one parked hash per level:
//   s.leaf(i)     cur = leaf hash i (the zero hash for i >= k)
//   s.emit(kind)  append (kind, cur) to the program (a Node's hash bytes are zero)
//   s.combine(l)  cur = SHA256(parked[l] || cur): the level-(l+1) node above cur
//   s.park_hash(l)     parked[l] = cur: a left child waits for its sibling
// At most one hash is parked per level 0 .. L-1, so the "stack" is L slots addressed by
// level.  After the pass cur is the root (the tx id).  The hashes computed are exactly
// those of the id computation: 2^L - 1 nodes.
template <class Inc, class Sink>
CG_HD void pmt_walk(uint32_t k, Inc&& inc, Sink& s) {
  if (k == 0) return;
  const uint32_t L = pmt_levels(k);
  const uint64_t kp = (uint64_t)1 << L;
  CG_NOUNROLL for (uint64_t i = 0; i < kp; ++i) {
    s.leaf(i);
    uint32_t l = 0;
    uint64_t idx = i;
    CG_NOUNROLL for (;;) {
      const int kind = pmt_emit_kind(inc, k, L, l, idx);
      if (kind >= 0) s.emit(kind);
      if (!(idx & 1)) break;  // a left child, or the root
      s.combine(l);
      idx >>= 1;
      ++l;
    }
    if (l < L) s.park_hash(l);
  }
}

// Program length of a tx: the pass with a sink that only counts.
struct PmtCountSink {
  uint32_t nodes = 0;
  CG_HDM void leaf(uint64_t) {}
  CG_HDM void emit(int) { ++nodes; }
  CG_HDM void combine(uint32_t) {}
  CG_HDM void park_hash(uint32_t) {}
};

template <class Inc>
CG_HD uint32_t pmt_node_count(uint32_t k, Inc&& inc) {
  PmtCountSink s;
  pmt_walk(k, inc, s);
  return s.nodes;
}

// The same length in closed form, from the tx's include bytes alone (what the host layout
// pass runs: O(k), not O(2^L) included-below tests).  A program with an included leaf is a
// full binary tree whose inner nodes are the Nodes, so it has 2 N + 1 entries, N = the number
// of distinct inner nodes above included leaves.  Taking the included indices in increasing
// order, index i shares with its predecessor p every ancestor at a level above the top bit
// of i ^ p, so it adds floor(log2(i ^ p)) new ones (the first adds all L).  Without an
// included leaf the program is the single Leaf(root).  The CPU tests hold the two counts
// against each other on every small shape.
CG_HD uint64_t pmt_node_count_mask(const uint8_t* include, uint32_t k) {
  if (k == 0) return 0;
  const uint32_t L = pmt_levels(k);
  uint64_t inner = 0;
  uint32_t prev = 0;
  bool any = false;
  for (uint32_t i = 0; i < k; ++i) {
    if (!include[i]) continue;
    uint32_t top = 0;
    for (uint32_t x = i ^ prev; x >>= 1;) ++top;
    inner += any ? top : L;
    prev = i;
    any = true;
  }
  return any ? 2 * inner + 1 : 1;
}

}  // namespace cg
