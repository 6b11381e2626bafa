/* fdt_keccak256.h -- Keccak-256 as one source for the host and the GPU: the
   hash of the secp256k1 precompile (fd_keccak256_hash, src/ballet/keccak256/
   fd_keccak256.c, called from fd_precompile_secp256k1_verify, src/flamenco/
   runtime/program/fd_precompiles.c:291,300).  Keccak[512] over a 1600-bit
   state (FIPS 202 section 3), rate 136 bytes, the original Keccak padding
   0x01 ... 0x80 (not SHA-3's 0x06), 32 bytes of output.

   Two forms over the one permutation:
     fdt_keccak256_absorb_block  block b of a message that is read through a
                                 reader (at(k): byte k of a payload), padding
                                 included; the device's form, one message per
                                 lane, the state in the lane's registers
     fdt_keccak256               a plain buffer to 32 bytes; the host's form
   Compiled by g++ into libfd_verify_tile.so (fdt_keccak256) and by hipcc
   into fdgpu_secp256k1.hip.

   Bounds: a reader is asked for message bytes only -- offsets below the
   message's size --, never for padding. */
#pragma once

#include <stdint.h>

#include "fdt_parse.h"

#if defined(__HIPCC__)
#define FDT_UNROLL _Pragma("unroll")
#define FDT_NOUNROLL _Pragma("unroll 1")
#else
#define FDT_UNROLL
#define FDT_NOUNROLL
#endif

#define FDT_KECCAK256_RATE 136u   /* bytes a block absorbs: (1600 - 2 * 256) / 8 */

/* the blocks of a message of sz bytes: the padding takes at least one byte */
FDT_HD uint32_t fdt_keccak256_block_cnt(uint32_t sz) { return sz / FDT_KECCAK256_RATE + 1u; }

FDT_HD uint64_t fdt_keccak_rotl(uint64_t x, uint32_t n) { return n ? (x << n) | (x >> (64u - n)) : x; }

/* the round constants of iota (FIPS 202 algorithm 5, 3.2.5) */
FDT_HD uint64_t fdt_keccak_rc(uint32_t round) {
  constexpr uint64_t rc[24] = {
      0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull,
      0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull,
      0x0000000080008009ull, 0x000000008000000aull, 0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull,
      0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800aull, 0x800000008000000aull,
      0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
  return rc[round];
}

/* Keccak-f[1600]: s[x + 5 y] is lane (x, y).  Every index below is a constant
   once the inner loops are unrolled, so the 25 lanes stay in registers; the
   round loop is kept. */
FDT_HD void fdt_keccak_f1600(uint64_t s[25]) {
  /* rho's offsets in the order pi visits the lanes from (1, 0) (3.2.2, 3.2.3) */
  constexpr uint32_t rot[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
  constexpr uint32_t pil[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
  FDT_NOUNROLL
  for (uint32_t round = 0; round < 24u; round++) {
    uint64_t c[5];
    FDT_UNROLL
    for (int x = 0; x < 5; x++) c[x] = s[x] ^ s[x + 5] ^ s[x + 10] ^ s[x + 15] ^ s[x + 20];         /* theta */
    FDT_UNROLL
    for (int x = 0; x < 5; x++) {
      const uint64_t d = c[(x + 4) % 5] ^ fdt_keccak_rotl(c[(x + 1) % 5], 1);
      FDT_UNROLL
      for (int y = 0; y < 25; y += 5) s[x + y] ^= d;
    }
    uint64_t t = s[1];                                                                                /* rho and pi */
    FDT_UNROLL
    for (int i = 0; i < 24; i++) {
      const uint64_t u = s[pil[i]];
      s[pil[i]] = fdt_keccak_rotl(t, rot[i]);
      t = u;
    }
    FDT_UNROLL
    for (int y = 0; y < 25; y += 5) {                                                                 /* chi */
      FDT_UNROLL
      for (int x = 0; x < 5; x++) c[x] = s[x + y];
      FDT_UNROLL
      for (int x = 0; x < 5; x++) s[x + y] = c[x] ^ (~c[(x + 1) % 5] & c[(x + 2) % 5]);
    }
    s[0] ^= fdt_keccak_rc(round);                                                                     /* iota */
  }
}

FDT_HD void fdt_keccak256_init(uint64_t s[25]) {
  FDT_UNROLL
  for (int i = 0; i < 25; i++) s[i] = 0;
}

/* Absorbs block b < fdt_keccak256_block_cnt(sz) of the message r.at(off +
   [0, sz)): its bytes [136 b, 136 b + 136), the padding's 0x01 behind the
   message's last byte and 0x80 on the last byte of the last block, then the
   permutation.  Lane w of the block is its bytes 8 w .. 8 w + 7, little
   endian (FIPS 202 appendix B.1). */
template <class Reader>
FDT_HD void fdt_keccak256_absorb_block(uint64_t s[25], Reader &r, uint64_t off, uint32_t sz, uint32_t b) {
  const uint32_t k0 = b * FDT_KECCAK256_RATE;
  const bool last = b + 1u == fdt_keccak256_block_cnt(sz);
  FDT_UNROLL
  for (uint32_t w = 0; w < FDT_KECCAK256_RATE / 8u; w++) {
    uint64_t v = 0;
    FDT_UNROLL
    for (uint32_t j = 0; j < 8u; j++) {
      const uint32_t k = k0 + 8u * w + j;
      uint32_t byte = 0;
      if (k < sz) byte = r.at(off + k);
      else if (k == sz) byte = 0x01u;
      v |= (uint64_t)byte << (8u * j);
    }
    if (last && w == FDT_KECCAK256_RATE / 8u - 1u) v ^= 0x80ull << 56;
    s[w] ^= v;
  }
  fdt_keccak_f1600(s);
}

/* digest byte k < 32 of a state all of whose blocks were absorbed */
FDT_HD uint32_t fdt_keccak256_digest_byte(const uint64_t s[25], uint32_t k) {
  const uint64_t v = k < 8u ? s[0] : k < 16u ? s[1] : k < 24u ? s[2] : s[3];
  return (uint32_t)(v >> (8u * (k & 7u))) & 0xFFu;
}

/* the plain-buffer form */
struct fdt_keccak_plain_reader {
  const uint8_t *p;
  FDT_HDM uint32_t at(uint64_t k) { return p[k]; }
};

FDT_HD void fdt_keccak256_core(const uint8_t *msg, uint64_t sz, uint8_t out[32]) {
  uint64_t s[25];
  fdt_keccak256_init(s);
  /* whole blocks in pieces a 32-bit size covers */
  while (sz >= FDT_KECCAK256_RATE * 0x1000000ull) {
    fdt_keccak_plain_reader r{msg};
    for (uint32_t b = 0; b < 0x1000000u; b++) fdt_keccak256_absorb_block(s, r, 0, 0xFFFFFFFFu, b);
    msg += FDT_KECCAK256_RATE * 0x1000000ull;
    sz -= FDT_KECCAK256_RATE * 0x1000000ull;
  }
  fdt_keccak_plain_reader r{msg};
  const uint32_t n = fdt_keccak256_block_cnt((uint32_t)sz);
  for (uint32_t b = 0; b < n; b++) fdt_keccak256_absorb_block(s, r, 0, (uint32_t)sz, b);
  for (uint32_t k = 0; k < 32u; k++) out[k] = (uint8_t)fdt_keccak256_digest_byte(s, k);
}
