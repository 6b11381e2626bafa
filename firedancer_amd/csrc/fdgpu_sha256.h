/* fdgpu_sha256.h -- one-message-per-lane SHA-256 (FIPS 180-4) on gfx950, for
   the shred path (fdgpu_shred.hip): the Merkle leaf hash of a shred (about
   1.1 KB behind a 26-byte constant prefix) and the node hashes of its
   inclusion proof (a fixed 66-byte, two-block message); and for the PoH path
   (fdgpu_poh.hip): the chain's hash of 32 bytes, the 65-byte leaf and branch
   of the 32-byte signature tree, the 64-byte mixin.

   The state and the 16-word message schedule live in VGPRs; rotates are
   v_alignbit_b32, the three-input xors, Ch and Maj one v_bitop3_b32 each.
   The message is never read byte by byte: a lane reads the 16-B aligned
   lines that cover its block (dwordx4 loads, whatever the message's
   alignment), realigns them in registers, and one v_perm_b32 per word does
   the byte shift and the big-endian swap at once.  Bytes past the message
   become the padding in registers; the loads themselves may run up to 80
   bytes past the message's end (the batch arena's FDGPU_ARENA_SLACK). */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef FDG_DEV
#define FDG_DEV __device__ __forceinline__
#endif

namespace fdgpu {

__constant__ static const uint32_t SHA256_K[64] = {
  0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
  0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
  0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
  0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
  0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
  0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
  0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
  0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
};

FDG_DEV uint32_t rotr32(uint32_t x, uint32_t r) { return __builtin_amdgcn_alignbit(x, x, r); }
/* v_bitop3_b32 truth tables (inputs weigh 0xF0, 0xCC, 0xAA): parity, choose, majority */
FDG_DEV uint32_t xor3_32(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
FDG_DEV uint32_t ch32(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }
FDG_DEV uint32_t maj32(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }

FDG_DEV void sha256_init(uint32_t (&h)[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

/* one block; w is consumed (the schedule is extended in place, 16 registers) */
FDG_DEV void sha256_compress(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  for (int r = 0; r < 64; r += 16) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
      if (r) {
        const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
        const uint32_t s0 = xor3_32(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
        const uint32_t s1 = xor3_32(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
        w[t] += s0 + w[(t + 9) & 15] + s1;
      }
      const uint32_t t1 = hh + xor3_32(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25)) + ch32(e, f, g) + SHA256_K[r + t] + w[t];
      const uint32_t t2 = xor3_32(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22)) + maj32(a, b, c);
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

/* NW big-endian words of the byte stream that starts at address q, from
   stream position s (a multiple of 4): the aligned lines covering them are
   read whole, shifted by the whole dwords of q's misalignment with two
   levels of selects, and each word is cut out of a dword pair by one v_perm
   whose selector carries the remaining 0..3 bytes and the byte swap */
template <int NW>
FDG_DEV void sha256_load_words(uint32_t (&w)[NW], const uint8_t *q, uint32_t s) {
  const uint32_t m16 = (uint32_t)((uintptr_t)q & 15u);
  const uint4 *v = (const uint4 *)(q - m16 + s);
  constexpr int NL = (NW + 1 + 3 + 3) / 4;        /* lines covering NW + 1 dwords shifted by up to 3 */
  uint32_t d[4 * NL + 2];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const uint4 x = v[i];
    d[4 * i] = x.x; d[4 * i + 1] = x.y; d[4 * i + 2] = x.z; d[4 * i + 3] = x.w;
  }
  d[4 * NL] = 0; d[4 * NL + 1] = 0;
  const bool k1 = (m16 & 4u) != 0, k2 = (m16 & 8u) != 0;
  uint32_t f[NW + 3];
#pragma unroll
  for (int i = 0; i < NW + 3; i++) {           /* values, not a choice between two addresses: the arrays stay registers */
    const uint32_t x0 = d[i], x1 = d[i + 1];
    f[i] = k1 ? x1 : x0;
  }
  const uint32_t sel = 0x00010203u + 0x01010101u * (m16 & 3u);
#pragma unroll
  for (int t = 0; t < NW; t++) {
    const uint32_t f0 = f[t], f1 = f[t + 1], f2 = f[t + 2], f3 = f[t + 3];
    w[t] = __builtin_amdgcn_perm(k2 ? f3 : f1, k2 ? f2 : f0, sel);
  }
}

/* the padding of a message of total bytes: word t of the block at stream
   position s keeps its bytes below total, takes the 0x80 after them, zeros
   beyond; the last block carries the bit length */
FDG_DEV void sha256_pad(uint32_t (&w)[16], uint32_t s, uint32_t total, bool last) {
#pragma unroll
  for (int t = 0; t < 16; t++) {
    const int32_t rem = (int32_t)total - (int32_t)(s + 4u * t);     /* message bytes in this word */
    if (rem < 4) {
      const uint32_t n = rem < 0 ? 0u : (uint32_t)rem;
      const uint32_t keep = n ? w[t] & (0xffffffffu << (32u - 8u * n)) : 0u;
      w[t] = rem >= 0 ? keep | (0x80000000u >> (8u * n)) : 0u;
    }
  }
  if (last) { w[14] = 0u; w[15] = total * 8u; }
}

FDG_DEV uint32_t sha256_blocks(uint32_t total) { return (total + 8u) / 64u + 1u; }

/* the 26 prefix bytes as the big-endian words 0..6 of the first block (word
   6: its upper half) */
struct sha256_prefix_t { uint32_t w[7]; };
constexpr sha256_prefix_t sha256_prefix_words(const char (&p)[27]) {
  sha256_prefix_t r{};
  for (int i = 0; i < 26; i++) r.w[i / 4] |= (uint32_t)(uint8_t)p[i] << (24 - 8 * (i % 4));
  return r;
}

/* SHA-256(prefix (26 B, PREFIX) || msg[0, msg_sz)), or of msg alone.  With
   the prefix the stream's base address is msg - 26: the words of the first
   block the prefix fills are overwritten, so what lies there is read but
   never used (the caller's 26 bytes before msg must be readable: a shred's
   leaf starts 64 bytes into it). */
template <bool PREFIX>
FDG_DEV void sha256_msg(uint32_t (&h)[8], const uint8_t *msg, uint32_t msg_sz, const sha256_prefix_t &pre) {
  const uint8_t *q = PREFIX ? msg - 26 : msg;
  const uint32_t total = msg_sz + (PREFIX ? 26u : 0u), nblk = sha256_blocks(total);
  sha256_init(h);
  for (uint32_t blk = 0; blk < nblk; blk++) {
    const uint32_t s = 64u * blk;
    uint32_t w[16];
    /* a block wholly past the message (only the length is left to write) reads the message's start instead */
    sha256_load_words<16>(w, q, s <= total ? s : 0u);
    if (PREFIX && blk == 0) {
#pragma unroll
      for (int t = 0; t < 6; t++) w[t] = pre.w[t];
      w[6] = pre.w[6] | (w[6] & 0xffffu);
    }
    sha256_pad(w, s, total, blk + 1u == nblk);
    sha256_compress(h, w);
  }
}

/* The node hash: SHA-256(prefix (26 B) || left[0,20) || right[0,20)), 66
   bytes, always two blocks.  left and right are five big-endian words each
   (the first five state words of a hash, or a proof node loaded as such).
   The first block's words 0..5 and half of 6 are the prefix's constants, the
   rest the nodes shifted by two bytes; the second block is right's last two
   bytes, the 0x80 and the length -- constants but for half a word. */
FDG_DEV void sha256_node(uint32_t (&h)[8], const uint32_t (&l)[5], const uint32_t (&r)[5], const sha256_prefix_t &pre) {
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 6; t++) w[t] = pre.w[t];
  w[6] = pre.w[6] | (l[0] >> 16);
#pragma unroll
  for (int t = 0; t < 4; t++) w[7 + t] = __builtin_amdgcn_alignbit(l[t], l[t + 1], 16);
  w[11] = __builtin_amdgcn_alignbit(l[4], r[0], 16);
#pragma unroll
  for (int t = 0; t < 4; t++) w[12 + t] = __builtin_amdgcn_alignbit(r[t], r[t + 1], 16);
  sha256_init(h);
  sha256_compress(h, w);
  w[0] = (r[4] << 16) | 0x8000u;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = 66u * 8u;
  sha256_compress(h, w);
}

/* ---- the PoH path (fdgpu_poh.hip) ---- */

/* One block from the initial state with every round unrolled: the round
   constants become literals, and whatever part of the state and of the
   schedule depends only on constant message words is folded at compile time.
   h receives the digest words. */
FDG_DEV void sha256_compress_unrolled(uint32_t (&h)[8], uint32_t (&w)[16]) {
  constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                              0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t a = IV[0], b = IV[1], c = IV[2], d = IV[3], e = IV[4], f = IV[5], g = IV[6], hh = IV[7];
#pragma unroll
  for (int r = 0; r < 64; r++) {
    const int t = r & 15;
    if (r >= 16) {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint32_t s0 = xor3_32(rotr32(w15, 7), rotr32(w15, 18), w15 >> 3);
      const uint32_t s1 = xor3_32(rotr32(w2, 17), rotr32(w2, 19), w2 >> 10);
      w[t] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t t1 = hh + xor3_32(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25)) + ch32(e, f, g) + SHA256_K[r] + w[t];
    const uint32_t t2 = xor3_32(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22)) + maj32(a, b, c);
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] = IV[0] + a; h[1] = IV[1] + b; h[2] = IV[2] + c; h[3] = IV[3] + d;
  h[4] = IV[4] + e; h[5] = IV[5] + f; h[6] = IV[6] + g; h[7] = IV[7] + hh;
}

/* One step of the PoH chain: h = SHA-256(h as 32 bytes).  The 8 state words
   of one hash are the 8 message words of the next, so a chain stays in
   registers and never swaps bytes; words 8..15 of its single block are the
   padding (0x80000000, zeros, the length 256), constants the schedule is
   folded over. */
FDG_DEV void sha256_hash32(uint32_t (&h)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 8; t++) w[t] = h[t];
  w[8] = 0x80000000u;
#pragma unroll
  for (int t = 9; t < 15; t++) w[t] = 0u;
  w[15] = 256u;
  sha256_compress_unrolled(h, w);
}

/* SHA-256(prefix (1 B) || m[0,64)), 65 bytes, always two blocks: the Merkle
   leaf (prefix 0, m a signature loaded with sha256_load_words) and branch
   (prefix 1, m two 32-byte nodes) of the 32-byte tree.  m is 16 big-endian
   words.  The first block is m shifted by one byte behind the prefix; the
   second is m's last byte, the 0x80 and the length -- constant but for that
   byte. */
FDG_DEV void sha256_hash65(uint32_t (&h)[8], uint32_t prefix, const uint32_t (&m)[16]) {
  uint32_t w[16];
  w[0] = (prefix << 24) | (m[0] >> 8);
#pragma unroll
  for (int t = 1; t < 16; t++) w[t] = __builtin_amdgcn_alignbit(m[t - 1], m[t], 8);
  sha256_init(h);
  sha256_compress(h, w);
  w[0] = (m[15] << 24) | 0x00800000u;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = 65u * 8u;
  sha256_compress(h, w);
}

/* The PoH mixin: h = SHA-256(h[32] || m[32]), 64 bytes, two blocks, the
   second one the padding alone */
FDG_DEV void sha256_mix64(uint32_t (&h)[8], const uint32_t (&m)[8]) {
  uint32_t w[16];
#pragma unroll
  for (int t = 0; t < 8; t++) { w[t] = h[t]; w[8 + t] = m[t]; }
  sha256_init(h);
  sha256_compress(h, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int t = 1; t < 15; t++) w[t] = 0u;
  w[15] = 64u * 8u;
  sha256_compress(h, w);
}

}  // namespace fdgpu
