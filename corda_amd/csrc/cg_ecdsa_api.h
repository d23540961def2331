// Host-side interface of the ECDSA (secp256k1 / secp256r1) kernels (K2-K4).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cg {

struct EcdsaConsts;  // per-context: generator tables + scratch

// Device-resident SoA subset of one curve (see ecdsa_kernels.hip for the layout).
struct EcdsaBatch {
  uint32_t n = 0;
  int scheme = 0;
  uint32_t* index = nullptr;    // positions in the full batch
  uint32_t* q = nullptr;        // [16][n]
  uint32_t* rs = nullptr;       // [16][n]
  uint32_t* der = nullptr;      // [n] DER status
  uint32_t* sig_len = nullptr;  // [n]
  uint64_t* msg_off = nullptr;  // [n]
  uint32_t* msg_len = nullptr;  // [n]
};

hipError_t ecdsa_consts_create(EcdsaConsts** out, hipStream_t s);
// test hook: secp256k1 elements whose index in the curve's subset is a multiple of m take
// the GLV split's full-length fallback (0: off)
void ecdsa_set_debug_glv(EcdsaConsts* c, uint32_t m);
void ecdsa_consts_free(EcdsaConsts* c);
// Stages one curve's subset into the SoA buffers of b (allocated by the caller:
// index[n] already uploaded, q[16n], rs[16n], der/sig_len/msg_len[n], msg_off[n]).
hipError_t ecdsa_batch_stage(const EcdsaBatch& b, const uint8_t* pk_raw_dev, size_t pk_stride,
                             const uint8_t* sig_raw_dev, size_t sig_stride, const uint32_t* sig_len_dev,
                             const uint64_t* msg_off_all_dev, const uint32_t* msg_len_all_dev, hipStream_t s);
// Scratch (one set per curve) is sized for min(n, chunk) elements; a batch is verified chunk by chunk:
// prep (key check, SHA-256, scalars, k*Q table) then msm (u1 G + u2 Q, x check).
hipError_t ecdsa_scratch(EcdsaConsts* c, int scheme, uint32_t n, uint32_t* chunk);
hipError_t ecdsa_launch_prep(const EcdsaBatch& b, EcdsaConsts* c, uint32_t base, uint32_t cnt, const uint8_t* arena,
                             uint32_t mode, hipStream_t s);
hipError_t ecdsa_launch_msm(const EcdsaBatch& b, EcdsaConsts* c, uint32_t base, uint32_t cnt, uint8_t* verdict,
                            hipStream_t s);
// K4 alone: strict DER -> rs [16][cap] LE limbs + status [cap] (0 ok, 1 range, 2 malformed)
hipError_t launch_der_parse(int scheme, const uint8_t* sig, size_t stride, const uint32_t* sig_len,
                            uint32_t fill_len, const uint32_t* idx, uint32_t n, uint32_t cap, uint32_t* rs,
                            uint32_t* der, hipStream_t s);

// Signing (K11, cg_ecdsa_sign.h).  The per-window tables of one curve (ecdsa_sign_tab_words()
// words, built once by launch_ecdsa_signtab_build); the signer's keys d [8][n_keys] LE limbs;
// one chunk of <= cap elements through scratch sized for cap: status[cap], ework[8 cap],
// xw[10 cap], invn / invp (ecdsa_sign_inv_words(cap, 8 / 10) words: they hold k, k^-1 and
// products of them, so the caller zeroes them before reuse).  Stage 0: hash, nonce, R = k G;
// stage 1: the two batched inversions; stage 2: r, s, DER -> sig (72-byte rows, zero past the
// signature), sig_len[i] (0 unless signed), status_out[i] (CG_SIGN_*).
struct EcdsaSignDev {
  int scheme = 0;
  const uint32_t* tab = nullptr;
  const uint32_t* key_index = nullptr;  // [n], or null: key 0
  const uint32_t* d = nullptr;
  uint32_t n_keys = 0;
  const uint8_t* arena = nullptr;
  const uint64_t* msg_off = nullptr;
  const uint32_t* msg_len = nullptr;
  uint32_t nonce_mode = 0;
  const uint32_t* k_rows = nullptr;  // [n] rows of 32 big-endian bytes (caller mode)
  uint32_t cap = 0;
  uint32_t *status = nullptr, *ework = nullptr, *xw = nullptr, *invn = nullptr, *invp = nullptr;
  uint8_t* sig = nullptr;
  uint32_t* sig_len = nullptr;
  uint8_t* status_out = nullptr;
};
size_t ecdsa_sign_tab_words();
size_t ecdsa_sign_inv_words(uint32_t cap, int words);
hipError_t launch_ecdsa_signtab_build(int scheme, uint32_t* tab, hipStream_t s);
// pub: 64-byte rows X || Y (big-endian), the verify key form
hipError_t launch_ecdsa_sign_keyexp(int scheme, const uint32_t* tab, const uint32_t* d, uint32_t n_keys, uint32_t* pub,
                                    hipStream_t s);
hipError_t launch_ecdsa_sign_stage(const EcdsaSignDev& d, uint32_t n, int stage, hipStream_t s);

}  // namespace cg
