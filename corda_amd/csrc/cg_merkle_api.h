// Host-side interface of the SHA-256 Merkle tx-id kernels (K5 leaves, K6 tree).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cg_pmt_build.h"

namespace cg {

// All pointers are device pointers (layout: merkle_kernels.hip).
// comp_tx[c] = owning tx of component c; for every signature s of tx t (sig_start
// may be null): sig_moff[s] = 32 t, sig_mlen[s] = 32.
hipError_t launch_tx_index(const uint32_t* comp_start, const uint32_t* sig_start, uint32_t n_tx, uint32_t* comp_tx,
                           uint64_t* sig_moff, uint32_t* sig_mlen, hipStream_t s);
// leaves[8c..8c+7] = leaf hash of component c for c in [c_begin, c_end); *err |= 1 when a
// component lies outside [0, arena_bytes).  nonces == nullptr: WireTransaction leaves
// (nonce from the tx salt, last component = privacy salt); otherwise FilteredLeaves
// leaves SHA256(ser_c || nonces[8c..8c+7]) (memory-order words).  With order (>= c_end -
// c_begin words) and hist (32 words) scratch, lanes take components grouped by length.
hipError_t launch_merkle_leaf(const uint8_t* arena, uint64_t arena_bytes, const uint64_t* comp_off,
                              const uint32_t* comp_len, const uint32_t* comp_start, const uint32_t* comp_tx,
                              const uint32_t* salts, const uint32_t* nonces, uint32_t c_begin, uint32_t c_end,
                              uint32_t* leaves, uint32_t* err, hipStream_t s, uint32_t* order = nullptr,
                              uint32_t* hist = nullptr);
// ids (8 words per tx, digest byte order) = Merkle root over the tx's leaves (in place).
hipError_t launch_merkle_tree(uint32_t* leaves, const uint32_t* comp_start, uint32_t n_tx, uint32_t* ids,
                              hipStream_t s);
// per tx: -1 all signatures ACCEPT, else index of the first non-ACCEPT one; -2 no signatures
hipError_t launch_first_bad(const uint8_t* verdict, const uint32_t* sig_start, uint32_t n_tx, int32_t* out,
                            hipStream_t s);

// Partial Merkle tree verdicts (status codes below); stack: 8 * max_depth * n words.
enum : uint8_t { kPmtTrue = 0, kPmtFalse = 1, kPmtNoLeaves = 2, kPmtMalformed = 3, kPmtHostCheck = 4 };
// (node kinds kPmtIncluded / kPmtLeaf / kPmtNode: cg_pmt_build.h)
constexpr uint32_t kPmtMaxLane = 256;
// Node-program well-formedness (status) and per-wave deepest stack (depth_w[(n + 63) / 64]).
hipError_t launch_pmt_scan(const uint32_t* node_start, const uint8_t* node_kind, uint32_t n, uint8_t* status,
                           uint32_t* depth_w, hipStream_t s);
hipError_t launch_pmt_eval(const uint32_t* node_start, const uint8_t* node_kind, const uint32_t* node_hash,
                           const uint32_t* comp_start, const uint32_t* leaves, const uint32_t* roots, uint32_t n,
                           uint32_t* stack, uint8_t* status, hipStream_t s);

// Partial Merkle tree construction (cg_ftx_build_batch; per-tx logic: cg_pmt_build.h).
// nonces[8 j ..] (digest byte order) = SHA256(salt_t || BE32(i)) of filtered component j =
// component fcomp_index[j] (< n_comp), the i-th of tx t = comp_tx[..].
hipError_t launch_pmt_nonce(const uint32_t* fcomp_index, uint32_t n_fcomp, uint32_t n_comp,
                            const uint32_t* comp_start, const uint32_t* comp_tx, const uint32_t* salts,
                            uint32_t* nonces, hipStream_t s);
// One lane per tx of [0, n) (comp_start / node_start / roots already offset to the first):
// the tx's post-order program into node_kind / node_hash at node_start[t] .., its root into
// roots[8 t ..] (zero for a tx without components).  leaves: K5's output, read only.
// inc_prefix[c] = number of included components before component c (n_comp + 1 entries).
// park: 8 * max(levels, 1) * stride words, stride >= n; levels >= the deepest tx's
// pmt_levels (a deeper tx is skipped: its nodes stay as they were).
hipError_t launch_pmt_build(const uint32_t* leaves, const uint32_t* comp_start, const uint32_t* inc_prefix,
                            const uint32_t* node_start, uint32_t n, uint32_t levels, uint32_t stride,
                            uint32_t* park, uint8_t* node_kind, uint32_t* node_hash, uint32_t* roots,
                            hipStream_t s);

}  // namespace cg
