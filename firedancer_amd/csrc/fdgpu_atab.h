/* fdgpu_atab.h -- the per-lane table entries of the verify chain as they are
   stored: a cached point (Y+X, Y-X, 2Z, 2dT) packed into 32 words, exactly
   one 128-B line, so a chain read touches one line and uses all of it (the
   unpacked entry's 160 B straddled two lines and used 62 % of them).

   A coordinate (10 limbs of 26, 25, 26, .. bits) is packed into 8 words:
   word j holds limb j in its low 26 (j even) or 25 (j odd) bits, which
   leaves 6, 7, 6, 7, .. spare high bits; limb 8 (26 bits) fills the spare
   bits of words 0..3 (6 + 7 + 6 + 7), limb 9 (25 bits) those of words 4..7.
   No limb crosses words in a way that needs a 64-bit shift: unpacking is 8
   v_and plus, for each of limbs 8 and 9, 4 shifts and 3 v_lshl_or (22
   full-rate instructions a coordinate), packing 14.

   Packing needs strictly tight limbs (limb i < 2^26 or 2^25); the products'
   and fe_carry's R bound is looser, so atab_store reduces each coordinate
   first (fe_tight; any representative of the residue serves, the chain only
   needs the value mod p).  Unpacked limbs are therefore strictly tight,
   which is inside the R bound the call sites of fdgpu_ge.h are annotated
   with.

   atab_store, atab_load, atab_pos and the LDS path (stage_entry,
   unstage_entry_signed) are the only code that knows the packed form: every
   other reader sees canonical-order limbs (Y+X, Y-X, 2Z, 2dT). */
#pragma once

#include <hip/hip_runtime.h>

#include "fdgpu_ge.h"
#include "fdgpu_internal.h"

namespace fdgpu {

/* Any limbs below 2^31 to strictly tight ones of the same residue.  A linear
   carry 0 -> 9 leaves limbs 0..8 tight; limb 9's excess c (< 2^6) re-enters
   limb 0 times 19, so the value is then below 2^255 + 19 c.  After the second
   pass limb 9 overflows (by one) only if that value reached 2^255: the rest
   is then below 19 c < 2^11, and adding 19 to limb 0 carries no further. */
FDG_DEV void fe_tight(fe &h) {
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int w = (i & 1) ? 25 : 26;
      h.v[i + 1] += h.v[i] >> w;
      h.v[i] &= (1u << w) - 1;
    }
    const uint32_t c = h.v[9] >> 25;
    h.v[9] &= (1u << 25) - 1;
    h.v[0] += 19u * c;
  }
}

/* strictly tight limbs -> 8 words */
FDG_DEV void fe_pack8(uint32_t (&w)[8], const fe &t) {
#pragma unroll
  for (int h = 0; h < 2; h++) {                 /* limb 8 over words 0..3, limb 9 over words 4..7 */
    const uint32_t s = t.v[8 + h];
    w[4 * h + 0] = t.v[4 * h + 0] | (s << 26);             /* bits 0..5 */
    w[4 * h + 1] = t.v[4 * h + 1] | ((s >> 6) << 25);      /* bits 6..12 */
    w[4 * h + 2] = t.v[4 * h + 2] | ((s >> 13) << 26);     /* bits 13..18 */
    w[4 * h + 3] = t.v[4 * h + 3] | ((s >> 19) << 25);     /* bits 19.. */
  }
}

/* 8 words -> 10 strictly tight limbs at q[0..9] */
FDG_DEV void fe_unpack8(uint32_t *q, const uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) q[j] = w[j] & ((j & 1) ? (1u << 25) - 1 : (1u << 26) - 1);
#pragma unroll
  for (int h = 0; h < 2; h++) {
    uint32_t s = w[4 * h + 3] >> 25;
    s = (s << 6) | (w[4 * h + 2] >> 26);
    s = (s << 7) | (w[4 * h + 1] >> 25);
    s = (s << 6) | (w[4 * h + 0] >> 26);
    q[8 + h] = s;
  }
}

/* Stored position of packed word j (0..7) of coordinate c (0 = Y+X, 1 = Y-X,
   2 = 2Z, 3 = 2dT): the words of Y+X and Y-X interleaved by pairs in the
   first four 16-B chunks -- chunk k = (Y+X words 2k, 2k+1, Y-X words 2k,
   2k+1) -- then 2Z (chunks 4, 5) and 2dT (chunks 6, 7) as they are.  A chain
   addition of -P reads Y+X and Y-X swapped: with pairs the swap is a
   per-lane 8-B offset of two ds_read_b64 (unstage_entry_signed) instead of
   per-word selects. */
__host__ __device__ constexpr int atab_pos(int c, int j) {
  return c >= 2 ? 8 * c + j : 4 * (j / 2) + 2 * c + (j % 2);
}

/* A table's entry 0 -- the identity in cached form (Y+X = Y-X = 1, 2Z = 2,
   2dT = 0), packed, in the stored word order -- is this one constant for
   every lane and table: digit-0 lookups read it (an L2 hit), and a lane's
   workspace holds only entries 1..8 of its tables. */
struct alignas(128) tab_ident_t { uint32_t w[FDGPU_PTAB_WORDS]; };
static __device__ const tab_ident_t g_tab_ident = {{1u, 0u, 1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 2u}};
static_assert(atab_pos(0, 0) == 0 && atab_pos(1, 0) == 2 && atab_pos(2, 0) == 16 && atab_pos(3, 7) == 31 &&
              atab_pos(0, 7) == 13 && atab_pos(1, 7) == 15, "the stored order (and the identity entry's)");

/* Entry |e| of a table whose (virtual) base is `tab` (entry k at tab + 32 k
   for k >= 1): the shared identity for e == 0. */
FDG_DEV const uint32_t *tab_entry(const uint32_t *tab, int e) {
  return e ? tab + (uint32_t)(e < 0 ? -e : e) * FDGPU_PTAB_WORDS : g_tab_ident.w;
}

FDG_DEV void atab_store(uint32_t *tab, uint32_t entry, const ge_cached &c) {
  uint4 *p = (uint4 *)(tab + entry * FDGPU_PTAB_WORDS);
  uint32_t o[FDGPU_PTAB_WORDS];
#pragma unroll
  for (int cc = 0; cc < 4; cc++) {
    fe t = cc == 0 ? c.YpX : cc == 1 ? c.YmX : cc == 2 ? c.Z2 : c.T2d;
    fe_tight(t);
    uint32_t w[8];
    fe_pack8(w, t);
#pragma unroll
    for (int j = 0; j < 8; j++) o[atab_pos(cc, j)] = w[j];
  }
#pragma unroll
  for (int q = 0; q < 8; q++) p[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
}

/* packed words in the stored order -> the entry's 40 limbs, canonical order */
FDG_DEV void atab_unpack(uint32_t (&q)[40], const uint32_t (&o)[FDGPU_PTAB_WORDS]) {
#pragma unroll
  for (int cc = 0; cc < 4; cc++) {
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = o[atab_pos(cc, j)];
    fe_unpack8(q + 10 * cc, w);
  }
}

FDG_DEV void atab_load(uint32_t (&q)[40], const uint32_t *tab, int e) {
  const uint4 *ent = (const uint4 *)tab_entry(tab, e);
  uint32_t o[FDGPU_PTAB_WORDS];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint4 v = ent[i];
    o[4 * i] = v.x; o[4 * i + 1] = v.y; o[4 * i + 2] = v.z; o[4 * i + 3] = v.w;
  }
  atab_unpack(q, o);
}

/* limb w (0..9) of coordinate c of the stored entry at ent, read in place */
FDG_DEV uint32_t atab_limb(const uint32_t *ent, int c, int w) {
  if (w < 8) return ent[atab_pos(c, w)] & ((w & 1) ? (1u << 25) - 1 : (1u << 26) - 1);
  const int b = 4 * (w - 8);
  uint32_t s = ent[atab_pos(c, b + 3)] >> 25;
  s = (s << 6) | (ent[atab_pos(c, b + 2)] >> 26);
  s = (s << 7) | (ent[atab_pos(c, b + 1)] >> 25);
  s = (s << 6) | (ent[atab_pos(c, b + 0)] >> 26);
  return s;
}

/* Table entries of the chain are staged through LDS by LDS-DMA
   (global_load_lds_dwordx4: no VGPR destination), issued at the start of a
   window and read back after its doublings, so no entry stays live in VGPRs
   across the doublings.  One wave-instruction moves 16 B for each of the 64
   lanes into 1 KiB of LDS (wave-uniform base + 16 B x lane): 8 of them move
   a packed entry (8 KiB per wave: FDGPU_STAGE_WAVE_WORDS). */
typedef __attribute__((address_space(3))) void lds_void_t;

FDG_DEV void stage_entry(uint32_t *lds_wave, const uint32_t *tab, int e) {
  const uint32_t *src = tab_entry(tab, e);
  constexpr int NCH = FDGPU_PTAB_WORDS / 4;
#pragma unroll
  for (int c = 0; c < NCH; c++)
    __builtin_amdgcn_global_load_lds((const void *)(src + 4 * c), (lds_void_t *)(lds_wave + 256 * c), 16, 0, 0);
}

/* The staged entry of a signed digit, unpacked: q[0..9] = Y+X of the digit's
   point (Y-X of the table's -kP when neg), q[10..19] the other, 2Z, 2dT as
   stored (2dT still to be negated when neg).  With the pair-interleaved
   entries the swap is the 8-B offset of two ds_read_b64 per pair chunk. */
FDG_DEV void unstage_entry_signed(uint32_t (&q)[40], const uint32_t *lds_wave, bool neg) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t *a = lds_wave + 4 * lane + (neg ? 2u : 0u), *b = lds_wave + 4 * lane + (neg ? 0u : 2u);
  uint32_t o[FDGPU_PTAB_WORDS];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const uint2 x = *(const uint2 *)(a + 256 * c), y = *(const uint2 *)(b + 256 * c);
    o[4 * c] = x.x; o[4 * c + 1] = x.y; o[4 * c + 2] = y.x; o[4 * c + 3] = y.y;
  }
#pragma unroll
  for (int c = 4; c < 8; c++) {
    const uint4 v = *(const uint4 *)(lds_wave + 256 * c + 4 * lane);
    o[4 * c] = v.x; o[4 * c + 1] = v.y; o[4 * c + 2] = v.z; o[4 * c + 3] = v.w;
  }
  atab_unpack(q, o);
}

}  // namespace fdgpu
